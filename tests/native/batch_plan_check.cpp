// Invariants of the batch tile plan (csrc/batch_plan.h), checked on the CPU: see tests/test_batch_plan_cpu.py.
//   batch_plan_check M N K BM BN BK nb1 lim_m lim_n lim_k write_all nbins len...      (one length per outer batch)
// prints "ok <n_active> <n_listed> <max bin load> <min bin load> <sum of bin loads>" (loads in K-blocks, bin = slot % nbins) or what failed.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../comprehensive-transformer-tts_amd/csrc/batch_plan.h"

#define FAIL(...) do { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); return 1; } while (0)

static std::vector<int32_t> build(const BatchPlanGeom& g, const std::vector<int32_t>& lens) {      // what batch_tile_map_kernel does
  const int n_items = (int)batch_plan_items(g), tiles = n_items / g.nbatch;
  std::vector<int32_t> map(BATCH_PLAN_HDR + n_items, -1);
  for (int i = 0; i < n_items; ++i) {
    const int z = i / tiles, tile = i - z * tiles;
    int n_active;
    const int slot = batch_plan_slot(g, lens.data(), z, tile, n_active);
    if (slot < 0 || slot >= n_items) { map[0] = -2; return map; }
    map[BATCH_PLAN_HDR + slot] = batch_plan_pack(z, tile);
    if (i == 0) { map[0] = n_active; map[1] = batch_plan_listed(g, n_active); map[2] = n_items; map[3] = batch_plan_key(g); }
  }
  return map;
}

int main(int argc, char** argv) {
  if (argc < 14) FAIL("usage");
  int a[12];
  for (int i = 0; i < 12; ++i) a[i] = std::atoi(argv[1 + i]);
  std::vector<int32_t> lens;
  for (int i = 13; i < argc; ++i) lens.push_back(std::atoi(argv[i]));
  BatchPlanGeom g{a[0], a[1], a[2], a[3], a[4], a[5], (int)lens.size() * a[6], a[6], a[7], a[8], a[9], a[10], a[11]};
  if (!batch_plan_fits(g)) FAIL("does not fit");
  const std::vector<int32_t> map = build(g, lens);
  if (map[0] == -2) FAIL("slot out of range");
  if (map != build(g, lens)) FAIL("two builds differ");
  const int n_items = (int)batch_plan_items(g), tiles_n = batch_plan_tiles_n(g), tiles = n_items / g.nbatch;
  const int n_active = map[0], n_listed = map[1];
  if (map[2] != n_items || n_listed != (g.write_all ? n_items : n_active)) FAIL("header");
  // every (batch, tile) exactly once; classes in order: active slots [0, n_active), the rest after them in plain order
  std::vector<char> seen(n_items, 0);
  long last_rest = -1;
  std::vector<long> bins(g.nbins, 0);
  for (int s = 0; s < n_items; ++s) {
    if (map[BATCH_PLAN_HDR + s] < 0) FAIL("slot %d empty", s);
    int z, tile;
    batch_plan_unpack(map[BATCH_PLAN_HDR + s], z, tile);
    if (z < 0 || z >= g.nbatch || tile < 0 || tile >= tiles) FAIL("slot %d: item (%d, %d)", s, z, tile);
    if (seen[z * tiles + tile]++) FAIL("item (%d, %d) twice", z, tile);
    const int L = lens[z / g.nb1];
    const int Mv = g.lim_m && L < g.M ? L : g.M, Nv = g.lim_n && L < g.N ? L : g.N, Kv = g.lim_k && L < g.K ? L : g.K;
    const bool active = (tile / tiles_n) * g.BM < Mv && (tile % tiles_n) * g.BN < Nv;      // the kernel's own test
    if (active != (s < n_active)) FAIL("slot %d: active item on the wrong side of n_active = %d", s, n_active);
    if (active) bins[s % g.nbins] += (Kv + g.BK - 1) / g.BK;
    else {
      if ((long)z * tiles + tile <= last_rest) FAIL("slot %d: rest not in plain order", s);
      last_rest = (long)z * tiles + tile;
    }
  }
  // ranks: work non-increasing, ties by batch then tile
  long pw = 1L << 40, pz = -1, pt = -1;
  for (int p = 0; p < n_active; ++p) {
    const int s = batch_plan_snake(p, n_active, g.nbins);
    if (s < 0 || s >= n_active) FAIL("rank %d: slot %d", p, s);
    int z, tile;
    batch_plan_unpack(map[BATCH_PLAN_HDR + s], z, tile);
    const long w = batch_plan_batch(g, lens[z / g.nb1]).work;
    if (w > pw || (w == pw && (z < pz || (z == pz && tile <= pt)))) FAIL("rank %d out of order", p);
    pw = w; pz = z; pt = tile;
  }
  long mx = 0, mn = 1L << 40, sum = 0;
  for (long b : bins) { mx = b > mx ? b : mx; mn = b < mn ? b : mn; sum += b; }
  std::printf("ok %d %d %ld %ld %ld\n", n_active, n_listed, mx, mn, sum);
  return 0;
}
