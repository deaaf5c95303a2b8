// Tile order of a batched, length-limited GEMM launch (gemm.hip, Fetch::BufferPartial: the attention products), shared by the device
// code and the CPU test of its invariants (tests/test_batch_plan_cpu.py compiles this header with g++).
//
// Item = one BM x BN output tile of one batch z (z = z0 * nb1 + z1; the batch's valid length is lens[z0]).  In plain block order item
// (z, tile) runs as workgroup z * tiles + tile, and the hardware deals consecutive workgroups over the compute units: the valid tiles of
// every utterance are its FIRST m-tiles, so the units that get low m-tiles carry the long K loops of several batches and the units that
// get high m-tiles carry one, or nothing.  The plan is a permutation slot <-> item in classes:
//   * ACTIVE items (row0 < Mv && col0 < Nv) first, sorted by work = ceil(Kv / BK) descending, then batch, then tile ascending, and
//     dealt in snake order over `nbins` bins (the CU count): rank p of layer p / nbins goes to the layer's slot p % nbins, counted from
//     the layer's other end in odd layers - the bin that got the heaviest item of one layer gets the lightest of the next.  A partial
//     last layer is reversed inside its own slots, so the active items fill exactly the slots [0, n_active);
//   * the REST after them in plain order: tiles that a "write everything" launch zero-fills (listed: n_listed = n_items), or that have
//     nothing to do at all (not listed: n_listed = n_active; workgroups from n_listed on exit at once).  Every tile of the grid lies
//     inside the batch's hard M x N block, so one launch has only one kind of rest.
// The plan changes WHERE an item runs, never what it computes.  Per-CU load in K-blocks of O = P V on the canonical fs2 batch (776
// active tiles, mean 76.1): plain order max 102, this order max 88 (uniform lengths: max = mean).
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#define BP_HD __host__ __device__ __forceinline__
#else
#define BP_HD inline
#endif

struct BatchPlanGeom {
  int M, N, K;                   // hard extents of one batch
  int BM, BN, BK;                // tile
  int nbatch, nb1;               // nb0 * nb1 batches; batch z reads lens[z / nb1]
  int lim_m, lim_n, lim_k;       // which extents the batch's length cuts
  int write_all;                 // 1: the launch zero-fills what lies outside the limits (split_overwrite)
  int nbins;                     // bins of the snake deal
};

// map layout: [0] n_active, [1] n_listed, [2] n_items, [3] batch_plan_key, then one packed item per slot
constexpr int BATCH_PLAN_HDR = 4;

BP_HD int batch_plan_tiles_m(const BatchPlanGeom& g) { return (g.M + g.BM - 1) / g.BM; }
BP_HD int batch_plan_tiles_n(const BatchPlanGeom& g) { return (g.N + g.BN - 1) / g.BN; }
BP_HD long batch_plan_items(const BatchPlanGeom& g) { return (long)g.nbatch * batch_plan_tiles_m(g) * batch_plan_tiles_n(g); }

// an item is one word, batch << 16 | tile; a slot costs a walk over all batches (batch_plan_slot)
BP_HD bool batch_plan_fits(const BatchPlanGeom& g) {
  const long tiles = (long)batch_plan_tiles_m(g) * batch_plan_tiles_n(g);
  return g.nbatch >= 1 && g.nb1 >= 1 && g.nbins >= 1 && tiles >= 1 && tiles <= 65536 && g.nbatch <= 32767 &&
         tiles * g.nbatch * g.nbatch <= (1L << 26);
}
BP_HD int32_t batch_plan_pack(int z, int tile) { return (int32_t)((z << 16) | tile); }
BP_HD void batch_plan_unpack(int32_t e, int& z, int& tile) { z = (int)((uint32_t)e >> 16); tile = e & 0xFFFF; }

// what a launch must agree on with its map besides n_items (a map built for another geometry is not used: plain order)
BP_HD int32_t batch_plan_key(const BatchPlanGeom& g) {
  return (int32_t)((g.lim_m & 1) | (g.lim_n & 1) << 1 | (g.lim_k & 1) << 2 | (g.write_all & 1) << 3 | (batch_plan_tiles_n(g) & 0xFFF) << 4 |
                   (g.BM & 0xFF) << 16 | (g.BN & 0xFF) << 24);
}

struct BatchPlanBatch {
  int work;            // K-blocks of an active tile
  int act_m, act_n;    // active m-tiles x active n-tiles: the FIRST ones
};

BP_HD BatchPlanBatch batch_plan_batch(const BatchPlanGeom& g, int L) {
  const int Mv = g.lim_m && L < g.M ? L : g.M, Nv = g.lim_n && L < g.N ? L : g.N, Kv = g.lim_k && L < g.K ? L : g.K;
  BatchPlanBatch b;
  b.work = Kv > 0 ? (Kv + g.BK - 1) / g.BK : 0;
  b.act_m = Mv > 0 ? (Mv + g.BM - 1) / g.BM : 0;
  b.act_n = Nv > 0 ? (Nv + g.BN - 1) / g.BN : 0;
  if (b.act_m == 0 || b.act_n == 0) b.act_m = b.act_n = 0;
  return b;
}

// slot of rank p among n_active: the snake deal
BP_HD int batch_plan_snake(int p, int n_active, int nbins) {
  const int layer = p / nbins, r = p - layer * nbins;
  const int width = n_active - layer * nbins < nbins ? n_active - layer * nbins : nbins;
  return layer * nbins + ((layer & 1) ? width - 1 - r : r);
}

// The slot of item (z, tile), and the launch's number of active items.  Pure, O(nbatch).
BP_HD int batch_plan_slot(const BatchPlanGeom& g, const int32_t* lens, int z, int tile, int& n_active) {
  const int tiles_n = batch_plan_tiles_n(g), tiles = batch_plan_tiles_m(g) * tiles_n;
  const BatchPlanBatch me = batch_plan_batch(g, lens[z / g.nb1]);
  int act_before = 0, rest_before = 0, total = 0;       // active items of the batches sorted before z; inactive ones of the batches < z
  for (int y = 0; y < g.nbatch; ++y) {
    const BatchPlanBatch o = batch_plan_batch(g, lens[y / g.nb1]);
    const int a = o.act_m * o.act_n;
    total += a;
    if (o.work > me.work || (o.work == me.work && y < z)) act_before += a;
    if (y < z) rest_before += tiles - a;
  }
  n_active = total;
  const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
  // active tiles of this batch before `tile` in plain order
  const int act_in = (tm < me.act_m ? tm : me.act_m) * me.act_n + (tm < me.act_m ? (tn < me.act_n ? tn : me.act_n) : 0);
  if (tm < me.act_m && tn < me.act_n) return batch_plan_snake(act_before + act_in, total, g.nbins);
  return total + rest_before + (tile - act_in);
}

BP_HD int batch_plan_listed(const BatchPlanGeom& g, int n_active) { return g.write_all ? (int)batch_plan_items(g) : n_active; }
