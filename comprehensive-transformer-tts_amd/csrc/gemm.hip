// fp32 MFMA GEMM for gfx950 with implicit-im2col operand views and a fused epilogue: the tile-per-workgroup kernels.
//
// gemm_tile_kernel: 256 threads = 4 waves (2 x 2, or 4 x 1 for 32-column tiles); block tile BM x BN x BK, wave tile as 32 x 32 MFMA
// tiles of v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD = the fp32 roofline on CDNA4).  K is consumed BK at a time; inside a
// 32-deep sub-block the MFMA's two k-lanes (lane>>5) take k = h*16 + j so that a K-contiguous operand is fetched from LDS as four
// ds_read_b128 per 32-row tile (row stride 36 floats -> conflict-free 16-lane groups).  Global->LDS staging goes through registers
// (prefetch of K-block i+1 is issued before the MFMAs of block i), which lets the loader apply the conv time-boundary predicate and the
// batch/length limits for free.  ONE body serves every way of fetching the operands (Fetch: scalar or 16-byte pointer loads, buffer
// loads, buffer loads with per-batch limits); what a fetch policy changes besides its loaders is listed in FetchTraits.
// gemm_buf_k2_kernel (two wave groups split the reduction), gemm_x6_kernel and gemm_x6tn_kernel (fp32 products on the bf16 matrix pipe)
// have main loops of their own; their prologues and the split-K reduce use the same helpers: rows_in_padding (the padding rule),
// gemm_split_range (gemm_common.h: the K range of a split), batch_limits, xcd_tile_order, zero_tile and zero_outside_limits.
// Host side: tile_plan / gemm_route decide which kernel takes a descriptor, ctts_gemm launches it.
#include "ctts_common.h"
#include "gemm_common.h"
#include "batch_plan.h"
#include <stdlib.h>
#include <type_traits>

namespace {

#ifndef CTTS_BK
#define CTTS_BK 32
#endif
#ifndef CTTS_GEMM_WAVES
#define CTTS_GEMM_WAVES 2
#endif
constexpr int BK = CTTS_BK;       // K elements staged per barrier pair (32 or 64); MFMA sub-blocks are always 32 deep
constexpr int KC_LD = BK + 4;     // row stride of K-contiguous operand tiles: 36 / 68 floats -> conflict-free b128 groups
constexpr int KCH = BK / 4;       // float4 chunks per tile row
static_assert(BK == 32 || BK == 64, "BK must be 32 or 64");

// ---- what every tile kernel of this file decides the same way ---------------------------------------------------------------------

// Rows first .. last of a (b, t) row space with row_T rows per utterance lie wholly in the padding of ONE utterance (beyond its length
// plus the halo).  Output rows there are defined as zero; reduction rows there contribute zero.
__device__ __forceinline__ bool rows_in_padding(const int32_t* row_lens, int row_T, int row_halo, int first, int last) {
  const int b0 = first / row_T;
  return b0 == last / row_T && (first - b0 * row_T) >= row_lens[b0] + row_halo;
}

// The extents of batch z0: M x N x K, each cut at the batch's valid length where the descriptor limits it (`apply`: the caller's
// kernel honours d.lens at all)
__device__ __forceinline__ void batch_limits(const ctts_gemm_desc& d, int z0, bool apply, int& Mv, int& Nv, int& Kv) {
  Mv = d.M; Nv = d.N; Kv = d.K;
  if (apply && d.lens) {
    const int L = d.lens[z0];
    if (d.lim_m) Mv = min(Mv, L);
    if (d.lim_n) Nv = min(Nv, L);
    if (d.lim_k) Kv = min(Kv, L);
  }
}

// What the tile order of a length-limited batched launch depends on (batch_plan.h); "write everything" as zero_outside_limits has it.
__host__ __device__ __forceinline__ BatchPlanGeom batch_plan_geom(const ctts_gemm_desc& d, int BM, int BN, int nbins) {
  return BatchPlanGeom{d.M, d.N, d.K, BM, BN, BK, d.nb0 * d.nb1, d.nb1, d.lim_m != 0, d.lim_n != 0, d.lim_k != 0,
                       d.split_overwrite != 0 && d.split_k <= 1, nbins};
}

// The K range of this workgroup: everything, or the share of its split (k_granule = `granule`).  false: an empty share, nothing to write.
__device__ __forceinline__ bool split_k_range(const ctts_gemm_desc& d, int Kv, int granule, int split, int& k_begin, int& k_end) {
  k_begin = 0; k_end = Kv;
  if (d.split_k > 1) {
    const GemmSplitRange s = gemm_split_range(Kv, d.split_k, granule, split);
    k_begin = s.k_begin; k_end = s.k_end;
    if (k_begin >= k_end) return false;
  }
  return true;
}

// XCD-contiguous tile order (bijective for any grid size): workgroup blockIdx.x runs on XCD blockIdx.x % 8, so each XCD gets a
// contiguous run of tiles (tiles that share an A panel hit the same L2).  scramble: the m-tiles are visited in an odd-prime stride
// permutation - with padded-row skipping the empty tiles of the short sequences would otherwise all land on the same XCD.
__device__ __forceinline__ void xcd_tile_order(int nwg, int tiles_n, bool scramble, int& wg, int& tm) {
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
  const int tiles_m = nwg / tiles_n;
  tm = wg / tiles_n;
  if (scramble) {
    const int P = (tiles_m % 37) ? 37 : ((tiles_m % 41) ? 41 : 43);
    tm = (int)(((long)tm * P) % tiles_m);
  }
}

// ctts_gemm_desc.tile_map is a device-built schedule, or this sentinel: plain blockIdx order (CTTS_NATURAL_ORDER / CTTS_TN_NATURAL)
__device__ __forceinline__ bool natural_order(const ctts_gemm_desc& d) { return d.tile_map == reinterpret_cast<const int32_t*>(1); }

// zeros into the [nrows, ncols] block of C at (row0, col0), and of Z where a forward epilogue would have stored it (whole workgroup)
__device__ __forceinline__ void zero_tile(const ctts_gemm_desc& d, float* C, int row0, int col0, int nrows, int ncols) {
  for (int e = threadIdx.x; e < nrows * ncols; e += 256) {
    const int r = e / ncols, c = e - r * ncols;
    C[(long)(row0 + r) * d.ldc + col0 + c] = 0.f;
    if (d.Z && !d.epi_bwd) d.Z[(long)(row0 + r) * d.ldz + col0 + c] = 0.f;
  }
}

// a tile whose rows row0 .. lie wholly in the padding of one utterance: zero-filled here - no operand traffic, no MFMA - and true
__device__ __forceinline__ bool padded_tile_zeroed(const ctts_gemm_desc& d, float* C, int row0, int col0, int BM, int ncols, int Mv) {
  const int last = min(row0 + BM, Mv) - 1;
  if (!rows_in_padding(d.row_lens, d.row_T, d.row_halo, row0, last)) return false;
  zero_tile(d, C, row0, col0, last - row0 + 1, ncols);
  return true;
}

// "write everything" (split_overwrite) on an unsplit batched launch with per-batch limits: what the BM x BN tile at (row0, col0) covers
// of the batch's [M, N] block but outside its limits Mv x Nv is WRITTEN as zero (the caller passes an uninitialised C: no fill launch per
// attention product; the epilogue never stores there).  whole: the tile lies beyond the limits altogether.
__device__ __forceinline__ void zero_outside_limits(const ctts_gemm_desc& d, float* C, int row0, int col0, int BM, int BN, int Mv, int Nv,
                                                    bool whole) {
  const int nrows = min(BM, d.M - row0), ncols = min(BN, d.N - col0);
  for (int e = threadIdx.x; e < nrows * ncols; e += 256) {
    const int r = e / ncols, c = e - r * ncols;
    if (whole || row0 + r >= Mv || col0 + c >= Nv) C[(long)(row0 + r) * d.ldc + col0 + c] = 0.f;
  }
}

// ---- operand loaders: one interface.  init(base, ld, ext0, ext_lim, conv view, tid) once per tile - the operand's (batch) base pointer
// and leading dimension, the tile's first row / column along the non-reduction extent and that extent's limit; load(k0, k_end, regs)
// fetches K-block k0 (cut at k_end) into staging registers; store(lds, regs) writes them to the LDS tile.
struct ConvView {
  int T, pad, cin;
};

// ---- K-contiguous operand tile: ROWS x BK, element (r,k) = P[r*ld + k]
template <int ROWS, bool CONV>
struct LoaderKC {
  static constexpr int NV = ROWS * BK / 4 / 256;
  const float* base;
  long ld;
  int row0, row_lim, kq, tid;
  ConvView cv;
  int trow[NV];
  __device__ __forceinline__ void init(const float* p, long ld_, int row0_, int row_lim_, ConvView cv_, int tid_) {
    base = CONV ? p - (long)cv_.pad * cv_.cin : p;      // conv: im2col row starts pad rows earlier
    ld = ld_; row0 = row0_; row_lim = row_lim_; cv = cv_; tid = tid_;
    kq = (tid % KCH) << 2;
    if (CONV) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        int gr = row0 + ((tid + i * 256) / KCH);
        trow[i] = gr % cv.T;
      }
    }
  }
  __device__ __forceinline__ void load(int k0, int k_end, float4 (&r)[NV]) const {
    const int gk = k0 + kq;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int gr = row0 + ((tid + i * 256) / KCH);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gr < row_lim && gk < k_end) {
        const float* p = base + (long)gr * ld + gk;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bool okq = (gk + q < k_end);
          if (CONV && okq) { int tt = trow[i] + (gk + q) / cv.cin - cv.pad; okq = (tt >= 0) && (tt < cv.T); }
          if (okq) e[q] = p[q];
        }
        v = make_float4(e[0], e[1], e[2], e[3]);
      }
      r[i] = v;
    }
  }
  __device__ __forceinline__ void store(float* s, const float4 (&r)[NV]) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int row = (tid + i * 256) / KCH;
      *reinterpret_cast<float4*>(s + row * KC_LD + kq) = r[i];
    }
  }
};

// ---- row-contiguous operand tile: BK x COLS, element (k,c) = P[k*ld + c]
template <int COLS, bool CONV>
struct LoaderRC {
  static constexpr int NV = COLS * BK / 4 / 256;
  static constexpr int LD = COLS + 4;
  const float* base;
  long ld;
  int col0, col_lim, tid;
  ConvView cv;
  __device__ __forceinline__ void init(const float* p, long ld_, int col0_, int col_lim_, ConvView cv_, int tid_) {
    base = CONV ? p - (long)cv_.pad * cv_.cin : p;
    ld = ld_; col0 = col0_; col_lim = col_lim_; cv = cv_; tid = tid_;
  }
  __device__ __forceinline__ void load(int k0, int k_end, float4 (&r)[NV]) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + i * 256;
      const int k = f / (COLS / 4);
      const int cq = (f % (COLS / 4)) << 2;
      const int gk = k0 + k, gc = col0 + cq;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gk < k_end && gc < col_lim) {
        const float* p = base + (long)gk * ld + gc;
        int trow = 0;
        if (CONV) trow = gk % cv.T;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bool okq = (gc + q < col_lim);
          if (CONV && okq) { int tt = trow + (gc + q) / cv.cin - cv.pad; okq = (tt >= 0) && (tt < cv.T); }
          if (okq) e[q] = p[q];
        }
        v = make_float4(e[0], e[1], e[2], e[3]);
      }
      r[i] = v;
    }
  }
  __device__ __forceinline__ void store(float* s, const float4 (&r)[NV]) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + i * 256;
      const int k = f / (COLS / 4);
      const int cq = (f % (COLS / 4)) << 2;
      *reinterpret_cast<float4*>(s + k * LD + cq) = r[i];
    }
  }
};


// ---------------------------------------------------------------------------------------------
// Branch-free loaders for the aligned case (Fetch::Vec): every 16-byte chunk is fetched UNCONDITIONALLY
// from an in-bounds address (invalid chunks read a safe dummy address: the operand's base) and the validity mask is
// applied only when the registers are written to LDS.  Nothing between the global_load and the
// ds_write consumes the loaded value, so hipcc keeps the loads in flight across the MFMA block
// (a select / branch join on the loaded value would force an s_waitcnt vmcnt(0) before the MFMAs).
// Requirements (checked on the host): leading dimensions, batch strides and base pointers are
// multiples of 4 floats and the contiguous extent (K, or M/N for row-contiguous operands) is a
// multiple of 4, so a chunk that starts inside the hard extent lies entirely inside it.
__device__ __forceinline__ float4 mask4(float4 v, int nv) {
  v.x = nv > 0 ? v.x : 0.f; v.y = nv > 1 ? v.y : 0.f; v.z = nv > 2 ? v.z : 0.f; v.w = nv > 3 ? v.w : 0.f;
  return v;
}

template <int ROWS, bool CONV>
struct VLoaderKC {
  static constexpr int NV = ROWS * BK / 4 / 256;
  const float* base; const float* safe;
  long ld;
  int row0, row_lim, kq, tid;
  ConvView cv;
  int trow[NV];
  int nval[NV];
  __device__ __forceinline__ void init(const float* p, long ld_, int row0_, int row_lim_, ConvView cv_, int tid_) {
    safe = p;
    base = CONV ? p - (long)cv_.pad * cv_.cin : p;
    ld = ld_; row0 = row0_; row_lim = row_lim_; cv = cv_; tid = tid_;
    kq = (tid % KCH) << 2;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int gr = row0 + ((tid + i * 256) / KCH);
      trow[i] = CONV ? gr % cv.T : 0;
      nval[i] = 0;
    }
  }
  __device__ __forceinline__ void load(int k0, int k_end, float4 (&r)[NV]) {
    const int gk = k0 + kq;
    int tap = 0;
    if (CONV) tap = gk / cv.cin - cv.pad;
    const int nk = min(4, k_end - gk);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int gr = row0 + ((tid + i * 256) / KCH);
      bool ok = (gr < row_lim) && (nk > 0);
      if (CONV) { const int tt = trow[i] + tap; ok = ok && (tt >= 0) && (tt < cv.T); }
      const float* p = ok ? base + (long)gr * ld + gk : safe;
      r[i] = *reinterpret_cast<const float4*>(p);
      nval[i] = ok ? nk : 0;
    }
  }
  __device__ __forceinline__ void store(float* s, const float4 (&r)[NV]) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int row = (tid + i * 256) / KCH;
      *reinterpret_cast<float4*>(s + row * KC_LD + kq) = mask4(r[i], nval[i]);
    }
  }
};

template <int COLS, bool CONV>
struct VLoaderRC {
  static constexpr int NV = COLS * BK / 4 / 256;
  static constexpr int LD = COLS + 4;
  const float* base; const float* safe;
  long ld;
  int col0, col_lim, tid;
  ConvView cv;
  int nval[NV];
  __device__ __forceinline__ void init(const float* p, long ld_, int col0_, int col_lim_, ConvView cv_, int tid_) {
    safe = p;
    base = CONV ? p - (long)cv_.pad * cv_.cin : p;
    ld = ld_; col0 = col0_; col_lim = col_lim_; cv = cv_; tid = tid_;
#pragma unroll
    for (int i = 0; i < NV; ++i) nval[i] = 0;
  }
  __device__ __forceinline__ void load(int k0, int k_end, float4 (&r)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + i * 256;
      const int k = f / (COLS / 4);
      const int cq = (f % (COLS / 4)) << 2;
      const int gk = k0 + k, gc = col0 + cq;
      const int nc = min(4, col_lim - gc);
      bool ok = (gk < k_end) && (nc > 0);
      if (CONV) { const int tt = gk % cv.T + gc / cv.cin - cv.pad; ok = ok && (tt >= 0) && (tt < cv.T); }
      const float* p = ok ? base + (long)gk * ld + gc : safe;
      r[i] = *reinterpret_cast<const float4*>(p);
      nval[i] = ok ? nc : 0;
    }
  }
  __device__ __forceinline__ void store(float* s, const float4 (&r)[NV]) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + i * 256;
      const int k = f / (COLS / 4);
      const int cq = (f % (COLS / 4)) << 2;
      *reinterpret_cast<float4*>(s + k * LD + cq) = mask4(r[i], nval[i]);
    }
  }
};

// ---------------------------------------------------------------------------------------------
// Buffer-descriptor loaders (Fetch::Buffer / BufferPartial).
// The operand is addressed as  SRD(base, 2 GiB window) + 32-bit byte offset.  A masked-out chunk simply
// gets the offset 0x80000000, which the hardware bounds check answers with zeros: no zero page, no select
// on the loaded data, no 64-bit pointer arithmetic - per chunk and K-block the address work is one add and
// (conv / K-tail only) one compare + v_cndmask.  Host guarantees every valid offset is < 2^31 bytes.
// PARTIAL: extents that are no multiple of 4 (per-batch limits) - the chunk that straddles the limit is cut when it is stored.
typedef unsigned int ctts_u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned CTTS_OOB = 0x80000000u;

__device__ __forceinline__ float4 buf_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned off) {
  ctts_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
  return *reinterpret_cast<float4*>(&v);
}

template <int ROWS, bool CONV, bool PARTIAL>
struct BLoaderKC {
  static constexpr int NV = ROWS * BK / 4 / 256;
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned boff[NV];      // byte offset of (row, kq) relative to the descriptor base, or CTTS_OOB
  int trow[NV];
  int kq, tid, T, cin, pad;
  int nk_cur;             // PARTIAL: valid elements of this thread's chunk in the staged K-block (same for all rows)
  __device__ __forceinline__ void init(const float* p, long ld, int row0, int row_lim, ConvView cv, int tid_) {
    rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, 0x7FFFFFFE, 0x00020000);
    tid = tid_; T = cv.T; cin = cv.cin; pad = cv.pad;
    kq = (tid % KCH) << 2;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int gr = row0 + ((tid + i * 256) / KCH);
      const long e = (long)(CONV ? gr - cv.pad : gr) * ld + kq;      // conv: im2col row starts pad rows earlier
      boff[i] = gr < row_lim ? (unsigned)(e * 4) : CTTS_OOB;
      trow[i] = CONV ? gr % cv.T : 0;
    }
    nk_cur = 4;
  }
  __device__ __forceinline__ void load(int k0, int k_end, float4 (&r)[NV]) {
    const int gk = k0 + kq;
    const bool kok = gk < k_end;                       // K tail: chunk fully masked, or (PARTIAL) cut at k_end
    if (PARTIAL) nk_cur = min(4, k_end - gk);
    const unsigned koff = (unsigned)k0 * 4u;
    int tap = 0;
    if (CONV) tap = gk / cin - pad;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      bool ok = kok && (boff[i] != CTTS_OOB);
      if (CONV) ok = ok && ((unsigned)(trow[i] + tap) < (unsigned)T);
      const unsigned off = ok ? boff[i] + koff : CTTS_OOB;   // select LAST: a wrapped (negative) boff plus an offset must never look valid
      r[i] = buf_load16(rsrc, off);
    }
  }
  __device__ __forceinline__ void store(float* s, const float4 (&r)[NV]) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int row = (tid + i * 256) / KCH;
      *reinterpret_cast<float4*>(s + row * KC_LD + kq) = PARTIAL ? mask4(r[i], nk_cur) : r[i];
    }
  }
};

template <int COLS, bool CONV, bool PARTIAL>
struct BLoaderRC {
  static constexpr int NV = COLS * BK / 4 / 256;
  static constexpr int LD = COLS + 4;
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned boff[NV];      // byte offset of (k_local row, column chunk) at k0 = 0, or CTTS_OOB
  int ctap[NV];           // CONV: gc / cin - pad (loop invariant)
  unsigned ldb4;          // row stride in bytes
  int tid, T;
  int ncol[NV];           // PARTIAL: valid elements of the chunk along the contiguous dim (loop invariant)
  __device__ __forceinline__ void init(const float* p, long ld, int col0, int col_lim, ConvView cv, int tid_) {
    rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, 0x7FFFFFFE, 0x00020000);
    tid = tid_; T = cv.T; ldb4 = (unsigned)(ld * 4);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + i * 256;
      const int k = f / (COLS / 4);
      const int gc = col0 + ((f % (COLS / 4)) << 2);
      const long e = (long)(CONV ? k - cv.pad : k) * ld + gc;
      boff[i] = gc < col_lim ? (unsigned)(e * 4) : CTTS_OOB;
      ctap[i] = CONV ? gc / cv.cin - cv.pad : 0;
      ncol[i] = PARTIAL ? min(4, col_lim - gc) : 4;
    }
  }
  __device__ __forceinline__ void load(int k0, int k_end, float4 (&r)[NV]) const {
    const unsigned k0off = (unsigned)k0 * ldb4;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int gk = k0 + (tid + i * 256) / (COLS / 4);
      unsigned off = boff[i] + k0off;
      bool ok = (boff[i] != CTTS_OOB) && (gk < k_end);
      if (CONV) ok = ok && ((unsigned)(gk % T + ctap[i]) < (unsigned)T);
      r[i] = buf_load16(rsrc, ok ? off : CTTS_OOB);
    }
  }
  __device__ __forceinline__ void store(float* s, const float4 (&r)[NV]) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + i * 256;
      *reinterpret_cast<float4*>(s + (f / (COLS / 4)) * LD + ((f % (COLS / 4)) << 2)) = PARTIAL ? mask4(r[i], ncol[i]) : r[i];
    }
  }
};

// ---- how the tile kernel fetches its operands, and everything else that follows from that choice
enum class Fetch {
  Scalar,           // dword pointer loads: any alignment, any extent (operands beyond the 2 GiB buffer window included)
  Vec,              // 16-byte pointer loads: aligned operands the buffer window does not cover
  Buffer,           // 16-byte buffer loads
  BufferPartial,    // ... with per-batch length limits (d.lens): the attention products
};

template <Fetch F>
struct FetchTraits {
  static constexpr bool kBuffer = F == Fetch::Buffer || F == Fetch::BufferPartial;
  // d.lens limits the extents of a batch: pointer fetch whenever d.lens is set; buffer fetch only in the partial variant, which
  // the launcher picks exactly when d.lens is set (the plain variant's loaders cannot cut a chunk) ...
  static constexpr bool kLensLimits = F != Fetch::Buffer;
  // ... so that variant takes the limits as given where the pointer kernels ask the descriptor
  static constexpr bool kLensGiven = F == Fetch::BufferPartial;
  // tile orders besides the XCD-contiguous one - device-built tile_map schedule, tile_group_n, the natural-order sentinel: only
  // tile_plan's buffer routes are set up with them; pointer fetch always uses the XCD remap
  static constexpr bool kTileOrders = kBuffer;
  // never the XCD-contiguous remap: the valid tiles of a short utterance are its FIRST rows / columns, and the remap would put all of
  // them on the first XCDs.  Plain blockIdx order (x = tile, z = batch) has the same fault one level down: consecutive workgroups are
  // dealt over the CUs, so with 32 m-tiles x 32 batches one CU holds tile j of batches z, z + 8, z + 16, z + 24 - the CUs with low j
  // carry four long K loops, those with high j one or none, and the launch lasts as long as its most loaded CU (O = P V with all
  // lengths 512 on T = 1024 operands: 40.5 us, the same work on T = 512 operands: 25.7 us).  With a plan in d.tile_map
  // (ctts_batch_tile_map, batch_plan.h) the workgroup's linear id picks (batch, tile) from a permutation that deals the active tiles,
  // heaviest first, evenly over the CUs; what a tile computes does not depend on where it runs.  Without one: plain order.
  static constexpr bool kNaturalOrder = F == Fetch::BufferPartial;
  // a tile the schedule lists as active skips the padded-tile test (the schedule was built with the same rule)
  static constexpr bool kTrustSchedule = kTileOrders;
  // the loaders cut partly valid chunks when they store to LDS (the others fetch only valid elements, or whole chunks)
  static constexpr bool kMaskAtStore = F == Fetch::Vec || F == Fetch::BufferPartial;
  // split-K: a padded tile's zeros go to the partial matrix of the workgroup's own split (buffer) or to the batch's first (pointer);
  // the reduce skips such tiles either way
  static constexpr bool kPadFillOwnSplit = kBuffer;
};

template <Fetch F, bool KC, int EXT, bool CONV>
using Loader = std::conditional_t<
    FetchTraits<F>::kBuffer,
    std::conditional_t<KC, BLoaderKC<EXT, CONV, FetchTraits<F>::kMaskAtStore>, BLoaderRC<EXT, CONV, FetchTraits<F>::kMaskAtStore>>,
    std::conditional_t<F == Fetch::Vec, std::conditional_t<KC, VLoaderKC<EXT, CONV>, VLoaderRC<EXT, CONV>>,
                       std::conditional_t<KC, LoaderKC<EXT, CONV>, LoaderRC<EXT, CONV>>>>;

// fragment fetch for one 32-wide MFMA tile: 16 k-steps, lane (l31, h) gets element k = h*16 + j
template <bool KC, int LD>
__device__ __forceinline__ void fetch_frag(const float* s, int ext0, int l31, int h, int ksub, float (&f)[16]) {
  if (KC) {
    const float4* p = reinterpret_cast<const float4*>(s + (ext0 + l31) * LD + ksub + h * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 v = p[q];
      f[4 * q + 0] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
    }
  } else {
    const float* p = s + (ksub + h * 16) * LD + ext0 + l31;
#pragma unroll
    for (int j = 0; j < 16; ++j) f[j] = p[j * LD];
  }
}

template <int BM, int BN, bool A_KC, bool B_KC, bool CONV, Fetch FETCH>
__global__ __launch_bounds__(256, CTTS_GEMM_WAVES) void gemm_tile_kernel(const ctts_gemm_desc d) {
  using FT = FetchTraits<FETCH>;
  // 4 waves as 2 x 2, or 4 x 1 for the narrow tile (BN = 32: outputs with N <= 32, e.g. the d_head = 32 attention gradients)
  constexpr int WAVES_N = BN >= 64 ? 2 : 1, WAVES_M = 4 / WAVES_N;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N, MT = WM / 32, NT = WN / 32;
  constexpr int A_LD = A_KC ? KC_LD : BM + 4;
  constexpr int B_LD = B_KC ? KC_LD : BN + 4;
  constexpr int A_SZ = A_KC ? BM * KC_LD : BK * (BM + 4);
  constexpr int B_SZ = B_KC ? BN * KC_LD : BK * (BN + 4);
  __shared__ __attribute__((aligned(16))) float smem[A_SZ + B_SZ];
  float* sA = smem;
  float* sB = smem + A_SZ;
  int z = blockIdx.z;
  const int split = blockIdx.y;                         // K split (grid.y = split_k, 1 when off); z = batch index
  const bool limited = FT::kLensLimits && (FT::kLensGiven || d.lens);      // per-batch valid lengths (attention over non-padded tokens only)
  // ---- which tile
  const int tiles_n = (d.N + BN - 1) / BN;
  int wg, tm;
  bool scheduled_active = false;
  if constexpr (FT::kNaturalOrder) {
    wg = blockIdx.x;
    if (d.tile_map && !natural_order(d)) {
      // length-balanced order: the workgroup's place in the launch names its item in the device-built plan.  A plan made for another
      // launch geometry is not followed (plain order); ids the plan does not list have nothing to do, not even zeros to write.
      const int32_t* plan = d.tile_map;
      const unsigned lin = blockIdx.z * gridDim.x + blockIdx.x;
      if (plan[2] == (int32_t)(gridDim.x * gridDim.z) && plan[3] == batch_plan_key(batch_plan_geom(d, BM, BN, 1))) {
        if (lin >= (unsigned)plan[1]) return;
        batch_plan_unpack(plan[BATCH_PLAN_HDR + lin], z, wg);
        if (z >= (int)gridDim.z || wg >= (int)gridDim.x) return;      // never an address from a damaged plan
      }
    }
    tm = wg / tiles_n;
  } else if (FT::kTileOrders && BM == 64 && A_KC && d.tile_map && !natural_order(d)) {
    // device-built schedule: active m-tiles first, natural workgroup order (round-robin over the XCDs)
    wg = blockIdx.x;
    int r = wg / tiles_n;
    if (d.tile_group_n > 0) {                     // XCD-grouped order (validated on the host): see ctts_gemm_desc.tile_group_n
      const int g = d.tile_group_n, ngroups = tiles_n / g, mways = 8 / ngroups;
      const int x = blockIdx.x & 7, i = blockIdx.x >> 3;
      r = (i / g) * mways + x / ngroups;
      wg = r * tiles_n + (x % ngroups) * g + i % g;
    }
    tm = d.tile_map[1 + r];
    scheduled_active = FT::kTrustSchedule && r < d.tile_map[0];
  } else if (FT::kTileOrders && natural_order(d)) {
    wg = blockIdx.x;
    tm = wg / tiles_n;
  } else {
    xcd_tile_order(gridDim.x, tiles_n, true, wg, tm);
  }
  const int z0 = z / d.nb1, z1 = z - z0 * d.nb1;
  int Mv, Nv, Kv;
  batch_limits(d, z0, limited, Mv, Nv, Kv);
  const int row0 = tm * BM, col0 = (wg % tiles_n) * BN;
  float* Cb = d.C + z0 * d.sC0 + z1 * d.sC1;
  // ---- tiles with nothing to multiply
  const bool zero_outside = limited && d.split_overwrite && d.split_k <= 1;
  if (row0 >= Mv || col0 >= Nv) {
    if (zero_outside && row0 < d.M && col0 < d.N) zero_outside_limits(d, Cb, row0, col0, BM, BN, Mv, Nv, true);
    return;
  }
  if (zero_outside && (row0 + BM > Mv || col0 + BN > Nv)) zero_outside_limits(d, Cb, row0, col0, BM, BN, Mv, Nv, false);
  float* Cs = Cb;
  if (d.split_k > 1) Cs += (long)split * d.M * d.ldc;      // split-K: C is the partial matrix P_split of the workspace (ctts_gemm rewrote the descriptor)
  if (A_KC && d.row_lens && !scheduled_active &&
      padded_tile_zeroed(d, FT::kPadFillOwnSplit ? Cs : Cb, row0, col0, BM, min(BN, Nv - col0), Mv)) return;
  int k_begin, k_end;
  if (!split_k_range(d, Kv, BK, split, k_begin, k_end)) return;

  // ---- operands
  ConvView cv{d.conv_T, d.conv_pad, d.conv_cin};
  ConvView nocv{1, 0, 1};
  constexpr bool CONV_A = CONV && A_KC;
  constexpr bool CONV_B = CONV && !A_KC && !B_KC;
  using LA = Loader<FETCH, A_KC, BM, CONV_A>;
  using LB = Loader<FETCH, B_KC, BN, CONV_B>;
  LA la; LB lb;
  la.init(d.A + z0 * d.sA0 + z1 * d.sA1, d.lda, row0, Mv, CONV_A ? cv : nocv, threadIdx.x);
  lb.init(d.B + z0 * d.sB0 + z1 * d.sB1, d.ldb, col0, Nv, CONV_B ? cv : nocv, threadIdx.x);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * WN;
  floatx16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // weight-gradient reductions run over (b,t) rows: K-blocks that lie entirely in the padding of one
  // sequence contribute exactly zero (dZ is zero there) and are skipped (block-uniform decision)
  constexpr bool KSKIP = !A_KC && !B_KC;
  auto kblock_active = [&](int k0) -> bool {
    if (!KSKIP || !d.row_lens) return true;
    return !rows_in_padding(d.row_lens, d.row_T, d.row_halo, k0, min(k0 + BK, k_end) - 1);
  };
  float4 ra[LA::NV], rb[LB::NV];
  bool act_cur = kblock_active(k_begin);
  if (act_cur) {
    la.load(k_begin, k_end, ra);
    lb.load(k_begin, k_end, rb);
    la.store(sA, ra);
    lb.store(sB, rb);
  }
  __syncthreads();
  for (int k0 = k_begin; k0 < k_end; k0 += BK) {
    const bool has_next = (k0 + BK) < k_end;
    const bool act_next = has_next && kblock_active(k0 + BK);
    if (act_next) {
      la.load(k0 + BK, k_end, ra);
      lb.load(k0 + BK, k_end, rb);
    }
    if (act_cur) {
#pragma unroll
      for (int ksub = 0; ksub < BK; ksub += 32) {
        float fa[MT][16], fb[NT][16];
#pragma unroll
        for (int i = 0; i < MT; ++i) fetch_frag<A_KC, A_LD>(sA, wm0 + i * 32, l31, h, ksub, fa[i]);
#pragma unroll
        for (int j = 0; j < NT; ++j) fetch_frag<B_KC, B_LD>(sB, wn0 + j * 32, l31, h, ksub, fb[j]);
#ifdef CTTS_GEMM_SETPRIO
        __builtin_amdgcn_s_setprio(CTTS_GEMM_SETPRIO);
#endif
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][kk], fb[j][kk], acc[i][j], 0, 0, 0);
#ifdef CTTS_GEMM_SETPRIO
        __builtin_amdgcn_s_setprio(0);
#endif
      }
    }
    if (KSKIP && !act_cur && !act_next) continue;   // nothing staged, nothing to publish: no barrier needed
    __syncthreads();
    if (act_next) {
      la.store(sA, ra);
      lb.store(sB, rb);
    }
    __syncthreads();
    act_cur = act_next;
  }
  gemm_epilogue_auto<MT, NT>(d, acc, Cs, z, row0, col0, wm0, wn0, l31, h, Mv, Nv);
}

// ---- fp32 GEMM on the BF16 matrix pipe (NT layout: both operands K-contiguous, conv view on A allowed) --------------------------
// v_mfma_f32_32x32x16_bf16 runs at 16x the rate of v_mfma_f32_32x32x2_f32 on gfx950.  Every fp32 operand is split EXACTLY into three
// bf16 pieces (x = hi + mid + lo, 8 significand bits each, each the round-to-nearest of what is left) once, on its way from the staging registers into LDS, and a
// product is the six cross terms  hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi  accumulated in fp32; the dropped terms are
// <= 2^-24 of the product in the worst case - ONE fp32 rounding - and 2^-29 in the median (|mid| <= 2^-8 |hi|, |lo| <= 2^-16 |hi|;
// tests/test_bf16_split_cpu.py; with truncated pieces the worst case was 2^-21),
// i.e. the products are fp32-class (measured: max error against float64 1.36e-5 where an fp32 FMA chain has 1.63e-5,
// tools/ubench/bf16x_split_gemm.hip; tests/test_kernels_gpu.py compares this kernel with float64 and with the fp32-MFMA kernels).
// Everything else is the tile kernel above: buffer loads with the im2col view, register staging, ONE LDS stage and two barriers per
// K-block (two workgroups per CU alternate), the same epilogues, the same zero-fill of wholly padded row tiles.  LDS: per operand three
// planes of [128 rows][32 bf16] = 64-byte rows with XOR-swizzled 16-byte chunks (conflict-free both ways) = 49,152 B per
// workgroup (LDS would take three per CU; the kernel's 188 VGPRs keep it at two waves per SIMD = two workgroups, which measured faster
// than three at 168 VGPRs with a spill).  The shader clock under this kernel is 1.8 - 1.9 GHz (2.39 under the fp32-MFMA kernels): DESIGN.md.
constexpr int X6_PROW = 64, X6_PLANE = 128 * X6_PROW;      // 64-byte rows, 16-byte chunks XOR-swizzled by (row >> 2) & 3 (see x6_chunk)
// physical 16-byte chunk of logical chunk c (0..3) in `row`: staging writes (8 lanes per row, 4 aligned rows per 256-byte beat) and
// fragment reads (16 consecutive rows, one chunk) both touch every bank exactly once per beat; no padding
__device__ __forceinline__ int x6_chunk(int row, int c) { return c ^ ((row >> 2) & 3); }
typedef __bf16 x6_bf16x8 __attribute__((ext_vector_type(8)));

typedef __bf16 x6_bf16x2 __attribute__((ext_vector_type(2)));
typedef float x6_floatx2 __attribute__((ext_vector_type(2)));
// two floats -> their bf16 roundings (to nearest even: v_cvt_pk_bf16_f32), packed low | high, and the exact remainders in place
__device__ __forceinline__ unsigned x6_round_pair(float& a, float& b) {
  const x6_floatx2 v = {a, b};
  const unsigned p = __builtin_bit_cast(unsigned, __builtin_convertvector(v, x6_bf16x2));
  a -= __uint_as_float(p << 16);                       // exact: a number minus its rounding to fewer bits
  b -= __uint_as_float(p & 0xFFFF0000u);
  return p;
}

__device__ __forceinline__ void x6_split_store(const float4 v, unsigned char* base) {      // 4 consecutive-K floats -> 8 bytes per plane
  float x0 = v.x, x1 = v.y, x2 = v.z, x3 = v.w;
  uint2 hi, mid, lo;
  hi.x = x6_round_pair(x0, x1);  hi.y = x6_round_pair(x2, x3);          // x = hi + r1
  mid.x = x6_round_pair(x0, x1); mid.y = x6_round_pair(x2, x3);         // r1 = mid + r2
  lo.x = x6_round_pair(x0, x1);  lo.y = x6_round_pair(x2, x3);          // r2 = lo exactly (<= 8 significant bits are left)
  *reinterpret_cast<uint2*>(base) = hi;
  *reinterpret_cast<uint2*>(base + X6_PLANE) = mid;
  *reinterpret_cast<uint2*>(base + 2 * X6_PLANE) = lo;
}

__device__ __forceinline__ floatx16 x6_mma(const ctts_u32x4 a, const ctts_u32x4 b, const floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x6_bf16x8, a), __builtin_bit_cast(x6_bf16x8, b), c, 0, 0, 0);
}

template <bool CONV>
__global__ __launch_bounds__(256, 2) void gemm_x6_kernel(const ctts_gemm_desc d) {
  static_assert(BK == 32, "the bf16 planes hold 32-deep K-blocks");
  constexpr int BM = 128, BN = 128, MT = 2, NT = 2;
  __shared__ __attribute__((aligned(16))) unsigned char smem[6 * X6_PLANE];       // A hi | mid | lo, B hi | mid | lo
  const int Mv = d.M, Nv = d.N, Kv = d.K;
  const int tiles_n = d.N / BN;
  int wg, tm;
  if (natural_order(d)) {
    wg = blockIdx.x; tm = wg / tiles_n;
  } else {          // as the tile kernel without a device-built schedule
    xcd_tile_order(gridDim.x, tiles_n, true, wg, tm);
  }
  const int row0 = tm * BM, col0 = (wg % tiles_n) * BN;
  float* Cb = d.C;
  if (d.row_lens && padded_tile_zeroed(d, Cb, row0, col0, BM, BN, Mv)) return;
  // the zero rule has 64-row granularity in the other kernels (and in the tile schedules built for them): when only the UPPER 64 rows of
  // this tile lie wholly in padding, the two waves that own them write zeros instead of their epilogue
  const bool pad_hi = d.row_lens && row0 + 64 < Mv && rows_in_padding(d.row_lens, d.row_T, d.row_halo, row0 + 64, min(row0 + BM, Mv) - 1);
  ConvView cv{d.conv_T, d.conv_pad, d.conv_cin};
  ConvView nocv{1, 0, 1};
  Loader<Fetch::Buffer, true, BM, CONV> la;
  Loader<Fetch::Buffer, true, BN, false> lb;
  la.init(d.A, d.lda, row0, Mv, CONV ? cv : nocv, threadIdx.x);
  lb.init(d.B, d.ldb, col0, Nv, nocv, threadIdx.x);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
  floatx16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float4 ra[4], rb[4];
  // staging: float4 i of this thread is row (tid + 256 i) / 8 = tid / 8 + 32 i, K offset (tid % 8) * 4 (BLoaderKC's chunking)
  // (rows 32 i apart share (row >> 2) & 3, so one swizzled offset serves all four staging rows / both MFMA row tiles)
  const int srow = threadIdx.x >> 3, sc8 = threadIdx.x & 7;
  unsigned char* st_a = smem + srow * X6_PROW + x6_chunk(srow, sc8 >> 1) * 16 + (sc8 & 1) * 8;
  unsigned char* st_b = st_a + 3 * X6_PLANE;
  // fragment of a 32-row MFMA tile: row l31, the 8 consecutive K values from h * 8 of the 16-deep step ks = logical chunk ks * 2 + h
  const unsigned char* fr_a = smem + (wm0 + l31) * X6_PROW;
  const unsigned char* fr_b = smem + 3 * X6_PLANE + (wn0 + l31) * X6_PROW;
  const int fc0 = x6_chunk(l31, h) * 16, fc1 = x6_chunk(l31, 2 + h) * 16;      // byte offsets of the fragment chunk for ks = 0, 1
  la.load(0, Kv, ra);
  lb.load(0, Kv, rb);
#pragma unroll
  for (int i = 0; i < 4; ++i) { x6_split_store(ra[i], st_a + 32 * i * X6_PROW); x6_split_store(rb[i], st_b + 32 * i * X6_PROW); }
  __syncthreads();
  for (int k0 = 0; k0 < Kv; k0 += BK) {
    {                                      // unconditional (the last block is fetched again): keeps the staging registers in registers
      const int kn = k0 + BK < Kv ? k0 + BK : k0;
      la.load(kn, Kv, ra);
      lb.load(kn, Kv, rb);
    }
    // all fragments of the K-block first (one exposed LDS round trip per block instead of one per 16-deep step), then the 48 MFMAs
    ctts_u32x4 fa[2][MT][3], fb[2][NT][3];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int p = 0; p < 3; ++p) fa[ks][i][p] = *reinterpret_cast<const ctts_u32x4*>(fr_a + p * X6_PLANE + 32 * i * X6_PROW + (ks ? fc1 : fc0));
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int p = 0; p < 3; ++p) fb[ks][j][p] = *reinterpret_cast<const ctts_u32x4*>(fr_b + p * X6_PLANE + 32 * j * X6_PROW + (ks ? fc1 : fc0));
    }
    // term-major order: consecutive MFMAs go to DIFFERENT accumulators (a chain of six on one accumulator waits for each result);
    // smallest terms first
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = x6_mma(fa[ks][i][PA[t]], fb[ks][j][PB[t]], acc[i][j]);
      }
    __syncthreads();                       // every wave has read the tile
#pragma unroll
    for (int i = 0; i < 4; ++i) { x6_split_store(ra[i], st_a + 32 * i * X6_PROW); x6_split_store(rb[i], st_b + 32 * i * X6_PROW); }
    __syncthreads();
  }
  if (pad_hi && wm0 == 64) {
    const int nrows = min(row0 + BM, Mv) - (row0 + 64);
    for (int e = lane; e < nrows * 64; e += 64) {
      const int r = e >> 6, c = e & 63;
      Cb[(long)(row0 + 64 + r) * d.ldc + col0 + wn0 + c] = 0.f;
      if (d.Z && !d.epi_bwd) d.Z[(long)(row0 + 64 + r) * d.ldz + col0 + wn0 + c] = 0.f;
    }
    return;
  }
  gemm_epilogue_auto<MT, NT>(d, acc, Cb, 0, row0, col0, wm0, wn0, l31, h, Mv, Nv);
}

// ---- the same arithmetic for WEIGHT GRADIENTS (TN layout: C[m][n] = sum_k A[k][m] B[k][n], both operands reduction-major, optional
// im2col view on B).  A bf16 MFMA fragment is 8 consecutive k of one row, which in memory lie a whole row apart: every thread owns ONE
// column (m or n) of the tile and reads 8 consecutive k of it with 8 dword loads (a wave still reads 256 contiguous bytes per k), splits
// the 8 values and stores 16 bytes per plane - the same LDS image as the NT kernel, so fragments, MFMA sequence and epilogue are shared.
// K-blocks that lie wholly in the padding of one utterance are skipped (their dZ rows are zero by construction); grid.y = split_k with
// ctts_gemm's ordered partial matrices.
template <bool CONV>
__global__ __launch_bounds__(256, 2) void gemm_x6tn_kernel(const ctts_gemm_desc d) {
  static_assert(BK == 32, "the bf16 planes hold 32-deep K-blocks");
  constexpr int BM = 128, BN = 128, MT = 2, NT = 2;
  __shared__ __attribute__((aligned(16))) unsigned char smem[6 * X6_PLANE];
  const int Mv = d.M, Nv = d.N, Kv = d.K;
  const int tiles_n = d.N / BN, split = blockIdx.y;
  int wg, tm;
  xcd_tile_order(gridDim.x, tiles_n, false, wg, tm);
  const int row0 = tm * BM, col0 = (wg % tiles_n) * BN;
  float* Cb = d.C;
  if (d.split_k > 1) Cb += (long)split * d.M * d.ldc;        // partial matrix P_split (ctts_gemm rewrote the descriptor)
  int k_begin, k_end;
  if (!split_k_range(d, Kv, BK, split, k_begin, k_end)) return;
  auto kblock_active = [&](int k0) -> bool {
    return !d.row_lens || !rows_in_padding(d.row_lens, d.row_T, d.row_halo, k0, min(k0 + BK, k_end) - 1);
  };
  auto next_active = [&](int k0) -> int { while (k0 < k_end && !kblock_active(k0)) k0 += BK; return k0; };
  const __amdgpu_buffer_rsrc_t ra_src = __builtin_amdgcn_make_buffer_rsrc((void*)d.A, 0, 0x7FFFFFFE, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb_src = __builtin_amdgcn_make_buffer_rsrc((void*)d.B, 0, 0x7FFFFFFE, 0x00020000);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
  // staging: thread -> column `scol` of both tiles, k octets og and og + 2 of the 32-deep block
  const int scol = threadIdx.x & 127, og = threadIdx.x >> 7;
  const unsigned a_col = (unsigned)(row0 + scol) * 4u, b_col = (unsigned)(col0 + scol) * 4u;
  const unsigned lda4 = (unsigned)(d.lda * 4), ldb4 = (unsigned)(d.ldb * 4);
  const int tapb = CONV ? (col0 + scol) / d.conv_cin - d.conv_pad : 0;      // im2col column = (tap, channel): the row shift of this column
  floatx16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float va[2][8], vb[2][8];
  auto gload = [&](int k0) {
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int kk0 = k0 + (og + 2 * o) * 8;
      const int t0 = CONV ? kk0 % d.conv_T + tapb : 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = kk0 + j;
        const bool ok = k < k_end;
        const unsigned offa = ok ? (unsigned)k * lda4 + a_col : CTTS_OOB;
        bool okb = ok;
        if (CONV) okb = okb && ((unsigned)(t0 + j) < (unsigned)d.conv_T);
        const unsigned offb = okb ? (unsigned)(CONV ? k - d.conv_pad : k) * ldb4 + b_col : CTTS_OOB;
        va[o][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra_src, offa, 0, 0));
        vb[o][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb_src, offb, 0, 0));
      }
    }
  };
  auto split_store8 = [&](const float (&xin)[8], unsigned char* base) {     // 8 consecutive k of one LDS row -> 16 bytes per plane
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = xin[i];
    ctts_u32x4 hi, mid, lo;
#pragma unroll
    for (int q = 0; q < 4; ++q) hi[q] = x6_round_pair(x[2 * q], x[2 * q + 1]);
#pragma unroll
    for (int q = 0; q < 4; ++q) mid[q] = x6_round_pair(x[2 * q], x[2 * q + 1]);
#pragma unroll
    for (int q = 0; q < 4; ++q) lo[q] = x6_round_pair(x[2 * q], x[2 * q + 1]);
    *reinterpret_cast<ctts_u32x4*>(base) = hi;
    *reinterpret_cast<ctts_u32x4*>(base + X6_PLANE) = mid;
    *reinterpret_cast<ctts_u32x4*>(base + 2 * X6_PLANE) = lo;
  };
  auto lstore = [&]() {
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      unsigned char* pa = smem + scol * X6_PROW + x6_chunk(scol, og + 2 * o) * 16;
      split_store8(va[o], pa);
      split_store8(vb[o], pa + 3 * X6_PLANE);
    }
  };
  const unsigned char* fr_a = smem + (wm0 + l31) * X6_PROW;
  const unsigned char* fr_b = smem + 3 * X6_PLANE + (wn0 + l31) * X6_PROW;
  const int fc0 = x6_chunk(l31, h) * 16, fc1 = x6_chunk(l31, 2 + h) * 16;
  int k_cur = next_active(k_begin);
  if (k_cur < k_end) {
    gload(k_cur);
    lstore();
  }
  __syncthreads();
  while (k_cur < k_end) {
    const int k_nxt = next_active(k_cur + BK);
    gload(k_nxt < k_end ? k_nxt : k_cur);                      // unconditional: keeps the staging registers out of scratch
    ctts_u32x4 fa[2][MT][3], fb[2][NT][3];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int p = 0; p < 3; ++p) fa[ks][i][p] = *reinterpret_cast<const ctts_u32x4*>(fr_a + p * X6_PLANE + 32 * i * X6_PROW + (ks ? fc1 : fc0));
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int p = 0; p < 3; ++p) fb[ks][j][p] = *reinterpret_cast<const ctts_u32x4*>(fr_b + p * X6_PLANE + 32 * j * X6_PROW + (ks ? fc1 : fc0));
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = x6_mma(fa[ks][i][PA[t]], fb[ks][j][PB[t]], acc[i][j]);
      }
    __syncthreads();
    lstore();
    __syncthreads();
    k_cur = k_nxt;
  }
  gemm_epilogue_auto<MT, NT>(d, acc, Cb, 0, row0, col0, wm0, wn0, l31, h, Mv, Nv);
}

// Under-filled launches (few output tiles, long reduction: the 2,048-row phoneme-level layers give 128 tiles of 64 x 64 on 256 CUs, each
// a chain of K / 32 staged K-blocks on one workgroup per CU): 32 x 64 tiles - twice the workgroups - and the reduction split in two INSIDE
// the workgroup.  Waves 0,1 (32 columns each) take the even 32-deep K-blocks, waves 2,3 the odd ones: one load / barrier round per 64
// of K, half as many rounds per workgroup, every SIMD of the chip in use.  The halves are added through LDS in a fixed order and waves
// 0,1 run the ordinary epilogue: any epilogue works (no atomics, no zero fill).  Padded 32-row tiles are zero-filled and skipped.
template <bool A_KC, bool B_KC, bool CONV>
__global__ __launch_bounds__(256, CTTS_GEMM_WAVES) void gemm_buf_k2_kernel(const ctts_gemm_desc d) {
  constexpr int BM = 32, BN = 64;
  constexpr int A_LD = A_KC ? KC_LD : BM + 4;
  constexpr int B_LD = B_KC ? KC_LD : BN + 4;
  constexpr int A_SZ = A_KC ? BM * KC_LD : BK * (BM + 4);
  constexpr int B_SZ = B_KC ? BN * KC_LD : BK * (BN + 4);
  static_assert(BK == 32, "the two-group kernel stages two 32-deep K-blocks per round");
  __shared__ __attribute__((aligned(16))) float smem[2 * (A_SZ + B_SZ)];       // [group][A | B]; reused for the final reduction
  const int z = blockIdx.z, split = blockIdx.y;
  const int z0 = z / d.nb1, z1 = z - z0 * d.nb1;
  const int Mv = d.M, Nv = d.N, Kv = d.K;
  const int tiles_n = (d.N + BN - 1) / BN;
  const int tm = blockIdx.x / tiles_n;
  const int row0 = tm * BM, col0 = (blockIdx.x - tm * tiles_n) * BN;
  if (row0 >= Mv || col0 >= Nv) return;
  float* Cb = d.C + z0 * d.sC0 + z1 * d.sC1;
  if (d.split_k > 1) Cb += (long)split * d.M * d.ldc;      // split-K: C is the partial matrix P_split of the workspace
  if (A_KC && d.row_lens && padded_tile_zeroed(d, Cb, row0, col0, BM, min(BN, Nv - col0), Mv)) return;
  int k_begin, k_end;
  if (!split_k_range(d, Kv, 2 * BK, split, k_begin, k_end)) return;
  ConvView cv{d.conv_T, d.conv_pad, d.conv_cin};
  ConvView nocv{1, 0, 1};
  constexpr bool CONV_A = CONV && A_KC;
  constexpr bool CONV_B = CONV && !A_KC && !B_KC;
  using LA = Loader<Fetch::Buffer, A_KC, BM, CONV_A>;
  using LB = Loader<Fetch::Buffer, B_KC, BN, CONV_B>;
  LA la; LB lb;
  la.init(d.A + z0 * d.sA0 + z1 * d.sA1, d.lda, row0, Mv, CONV_A ? cv : nocv, threadIdx.x);
  lb.init(d.B + z0 * d.sB0 + z1 * d.sB1, d.ldb, col0, Nv, CONV_B ? cv : nocv, threadIdx.x);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int grp = wave >> 1, wn0 = (wave & 1) * 32;
  float* sA = smem + grp * (A_SZ + B_SZ);
  float* sB = sA + A_SZ;
  floatx16 acc[1][1];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
  float4 ra[2][LA::NV], rb[2][LB::NV];
  auto load_round = [&](int k0) {                       // both 32-deep K-blocks of the round (the second may lie beyond k_end: zeros)
    la.load(k0, k_end, ra[0]);      lb.load(k0, k_end, rb[0]);
    la.load(k0 + BK, k_end, ra[1]); lb.load(k0 + BK, k_end, rb[1]);
  };
  auto store_round = [&]() {
    la.store(smem, ra[0]);                  lb.store(smem + A_SZ, rb[0]);
    la.store(smem + A_SZ + B_SZ, ra[1]);    lb.store(smem + 2 * A_SZ + B_SZ, rb[1]);
  };
  load_round(k_begin);
  store_round();
  __syncthreads();
  for (int k0 = k_begin; k0 < k_end; k0 += 2 * BK) {
    const bool has_next = (k0 + 2 * BK) < k_end;
    if (has_next) load_round(k0 + 2 * BK);
    {
      float fa[16], fb[16];
      fetch_frag<A_KC, A_LD>(sA, 0, l31, h, 0, fa);
      fetch_frag<B_KC, B_LD>(sB, wn0, l31, h, 0, fb);
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk], fb[kk], acc[0][0], 0, 0, 0);
    }
    __syncthreads();
    if (has_next) store_round();
    __syncthreads();
  }
  // waves 2,3 hand their half over through LDS (the operand tiles are dead: the loop's last barrier is behind every fragment read)
  float* red = smem + (wave & 1) * 1024 + lane;
  if (grp == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[r * 64] = acc[0][0][r];
  }
  __syncthreads();
  if (grp == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] += red[r * 64];
  }
  if (grp == 0) gemm_epilogue_auto<1, 1>(d, acc, Cb, z, row0, col0, 0, wn0, l31, h, Mv, Nv);
}

template <bool A_KC, bool B_KC, bool CONV>
int launch_buf_k2(const ctts_gemm_desc& d, hipStream_t st) {
  const int tiles = ((d.M + 31) / 32) * ((d.N + 63) / 64);
  const int nz = d.nb0 * d.nb1, ny = d.split_k > 1 ? d.split_k : 1;
  hipLaunchKernelGGL((gemm_buf_k2_kernel<A_KC, B_KC, CONV>), dim3(tiles, ny, nz), dim3(256), 0, st, d);
  CTTS_CHECK_LAUNCH("ctts_gemm(buf,k2)");
  return 0;
}

// The three instantiated operand layouts (NT, NN, TN), with or without a conv view: f(a_kc, b_kc, conv) gets them as compile-time
// constants.  WITH_CONV = false: the caller has no conv instantiations (its route never carries a conv view).
template <bool WITH_CONV, class F>
int for_layout(const ctts_gemm_desc& d, F f) {
  auto go = [&](auto a, auto b) {
    if constexpr (WITH_CONV) {
      if (d.conv_T > 0) return f(a, b, std::true_type{});
    }
    return f(a, b, std::false_type{});
  };
  if (d.a_kc && d.b_kc) return go(std::true_type{}, std::true_type{});
  if (d.a_kc && !d.b_kc) return go(std::true_type{}, std::false_type{});
  if (!d.a_kc && !d.b_kc) return go(std::false_type{}, std::false_type{});
  ctts_set_error("ctts_gemm: layout a_kc=0,b_kc=1 is not instantiated");
  return -1;
}

// One launch of the tile kernel.  Buffer fetch with per-batch length limits in force goes to the partial variant (no conv instantiations).
template <int BM, int BN, bool A_KC, bool B_KC, bool CONV, Fetch FETCH>
int launch_tile(const ctts_gemm_desc& d, hipStream_t st) {
  if constexpr (FETCH == Fetch::Buffer) {
    if (d.lens && (d.lim_m || d.lim_n || d.lim_k)) {
      if constexpr (!CONV) {
        return launch_tile<BM, BN, A_KC, B_KC, false, Fetch::BufferPartial>(d, st);
      } else {
        ctts_set_error("ctts_gemm: per-batch length limits together with a conv view are not supported");
        return -1;
      }
    }
  }
  const int tiles = ((d.M + BM - 1) / BM) * ((d.N + BN - 1) / BN);
  const int nz = d.nb0 * d.nb1, ny = d.split_k > 1 ? d.split_k : 1;
  hipLaunchKernelGGL((gemm_tile_kernel<BM, BN, A_KC, B_KC, CONV, FETCH>), dim3(tiles, ny, nz), dim3(256), 0, st, d);
  CTTS_CHECK_LAUNCH(FETCH == Fetch::BufferPartial ? "ctts_gemm(buf,partial)" : FETCH == Fetch::Buffer ? "ctts_gemm(buf)" : "ctts_gemm");
  return 0;
}

// buffer loaders need: no per-batch length limits and every operand element within 2 GiB of its (batch) base
bool buf_ok(const ctts_gemm_desc& d) {
  if (d.lens && (d.lim_m || d.lim_n || d.lim_k) && d.conv_T > 0) return false;
  const long a_ext = d.a_kc ? ((long)d.M * d.lda + d.K) : ((long)d.K * d.lda + d.M);
  const long b_ext = d.b_kc ? ((long)d.N * d.ldb + d.K) : ((long)d.K * d.ldb + d.N);
  return a_ext * 4 < 0x7FFF0000L && b_ext * 4 < 0x7FFF0000L;
}

// eligibility of the branch-free 16-byte loaders (see VLoaderKC)
bool chunks_ok(const ctts_gemm_desc& d) {          // every 4-float chunk along the contiguous dimension lies inside the operand or outside it
  const bool a_ext = d.a_kc ? (d.K % 4 == 0) : (d.M % 4 == 0);
  const bool b_ext = d.b_kc ? (d.K % 4 == 0) : (d.N % 4 == 0);
  return a_ext && b_ext;
}
bool vec_ok(const ctts_gemm_desc& d) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool strides = !((d.lda | d.ldb | d.sA0 | d.sA1 | d.sB0 | d.sB1) & 3);
  return strides && chunks_ok(d) && al16(d.A) && al16(d.B);
}

// one wave: stable partition of the m-tiles into active (first) and inactive, count in map[0]
__global__ __launch_bounds__(64) void row_tile_map_kernel(const int32_t* __restrict__ row_lens, int row_T, int row_halo, int M,
                                                            int32_t* __restrict__ map) {
  const int tiles = (M + 63) / 64, lane = threadIdx.x;
  auto inactive = [&](int tm) -> bool { return rows_in_padding(row_lens, row_T, row_halo, tm * 64, min(tm * 64 + 64, M) - 1); };
  int n_act = 0;
  for (int base = 0; base < tiles; base += 64) {
    const int tm = base + lane;
    const bool a = tm < tiles && !inactive(tm);
    const unsigned long long m = __ballot(a);
    if (a) map[1 + n_act + __popcll(m & ((1ULL << lane) - 1ULL))] = tm;
    n_act += __popcll(m);
  }
  int n_in = 0;
  for (int base = 0; base < tiles; base += 64) {
    const int tm = base + lane;
    const bool a = tm < tiles && inactive(tm);
    const unsigned long long m = __ballot(a);
    if (a) map[1 + n_act + n_in + __popcll(m & ((1ULL << lane) - 1ULL))] = tm;
    n_in += __popcll(m);
  }
  if (lane == 0) map[0] = n_act;
}

// The plan of batch_plan.h for one launch geometry, from the lengths on the device: thread i places item i.  map: BATCH_PLAN_HDR +
// n_items int32 (the host checked batch_plan_fits and the size).
__global__ __launch_bounds__(256) void batch_tile_map_kernel(const BatchPlanGeom g, const int32_t* __restrict__ lens, int32_t* __restrict__ map) {
  const int n_items = (int)batch_plan_items(g), tiles = n_items / g.nbatch;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_items; i += gridDim.x * 256) {
    const int z = i / tiles, tile = i - z * tiles;
    int n_active;
    const int slot = batch_plan_slot(g, lens, z, tile, n_active);
    map[BATCH_PLAN_HDR + slot] = batch_plan_pack(z, tile);
    if (i == 0) {
      map[0] = n_active;
      map[1] = batch_plan_listed(g, n_active);
      map[2] = n_items;
      map[3] = batch_plan_key(g);
    }
  }
}

// Second launch of a split-K GEMM: C[m, n] += alpha * (P_0 + P_1 + ... )[m, n] in split order (fixed: bit-reproducible), for the rows /
// columns / batches the GEMM kernels computed - per-batch length limits, tiles of padded rows (zero-filled by the GEMM, skipped here) and
// splits whose K range was empty (never written) follow the kernels' own predicates.  One thread per 4 columns, all splits' loads in flight.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const ctts_gemm_desc d, int BM, int kround) {
  const int z = blockIdx.z, z0 = z / d.nb1, z1 = z - z0 * d.nb1;
  int Mv, Nv, Kv;
  batch_limits(d, z0, true, Mv, Nv, Kv);
  const bool ow = d.split_overwrite != 0;      // C = alpha * sum (and ZERO outside the limits / in padded tiles) instead of C += : no pre-zeroed C
  const int nact = Kv > 0 ? gemm_split_range(Kv, d.split_k, kround, 0).nonempty : 0;
  if (nact == 0 && !ow) return;
  const long ldp = gemm_partial_ld(d.N);
  const int n4 = (int)(ldp >> 2);
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int m = (int)(e / n4), n = (int)(e - (long)m * n4) * 4;
  if (m >= d.M || n >= d.N) return;
  bool live = m < Mv && n < Nv && nact > 0;
  if (live && d.a_kc && d.row_lens) {          // the GEMM wrote no partials for whole tiles of padded rows (their result is defined as zero)
    const int row0 = m / BM * BM;
    if (rows_in_padding(d.row_lens, d.row_T, d.row_halo, row0, min(row0 + BM, Mv) - 1)) live = false;
  }
  if (!live && !ow) return;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float4* P = reinterpret_cast<const float4*>(gemm_partial_base(d, z, 0) + (long)m * ldp + n);
    const long sstride = (long)d.M * ldp / 4;          // P_s of a batch are consecutive [M, ldp] matrices
    for (int s = 0; s < nact; s += 8) {          // eight partials in flight, added in split order
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = (s + u < nact) ? P[(long)(s + u) * sstride] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < 8; ++u) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
    }
  }
  float* Cr = d.C + z0 * d.sC0 + z1 * d.sC1 + (long)m * d.ldc + n;
  const float al = d.alpha;
  const int ncols = ow ? d.N : Nv;              // overwrite mode also zeroes the columns between the batch's limit and N
  if (n + 4 <= Nv && ((reinterpret_cast<uintptr_t>(Cr) & 15) == 0)) {
    float4 c = ow ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<float4*>(Cr);
    c.x += al * a.x; c.y += al * a.y; c.z += al * a.z; c.w += al * a.w;
    *reinterpret_cast<float4*>(Cr) = c;
  } else {
    const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (n + q < ncols) Cr[q] = (ow ? 0.f : Cr[q]) + ((live && n + q < Nv) ? al * av[q] : 0.f);
  }
}

int splitk_reduce(const ctts_gemm_desc& d, int BM, int kround, hipStream_t st) {
  const long e = (long)d.M * (gemm_partial_ld(d.N) / 4);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((e + 255) / 256), 1, d.nb0 * d.nb1), dim3(256), 0, st, d, BM, kround);
  CTTS_CHECK_LAUNCH("ctts_gemm(split-K reduce)");
  return 0;
}
}  // namespace

extern "C" int ctts_row_tile_map(const int32_t* row_lens, int row_T, int row_halo, int M, int32_t* tile_map, void* stream) {
  CTTS_REQUIRE(row_lens && tile_map && row_T > 0 && M >= 0, "ctts_row_tile_map: bad arguments");
  hipLaunchKernelGGL(row_tile_map_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, row_lens, row_T, row_halo, M, tile_map);
  CTTS_CHECK_LAUNCH("ctts_row_tile_map");
  return 0;
}

// the length-limited batched launches run on 64 x 64 tiles (tile_plan: BUF64 -> Fetch::BufferPartial); bins = the CUs of the device
static BatchPlanGeom batch_map_geom(int nb0, int nb1, int M, int N, int K, int lim_m, int lim_n, int lim_k, int write_all) {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipDeviceProp_t prop;
    cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
              ? prop.multiProcessorCount : 256;
    cus = ctts_env_int("CTTS_BATCH_BINS", cus);          // tuning knob
    if (cus < 1) cus = 256;
  }
  return BatchPlanGeom{M, N, K, 64, 64, BK, nb0 * nb1, nb1, lim_m != 0, lim_n != 0, lim_k != 0, write_all != 0, cus};
}

extern "C" size_t ctts_batch_tile_map_ints(int nb0, int nb1, int M, int N) {
  if (nb0 < 1 || nb1 < 1 || M < 1 || N < 1 || (long)nb0 * nb1 > 32767) return 0;
  const BatchPlanGeom g = batch_map_geom(nb0, nb1, M, N, 1, 0, 0, 0, 0);
  return batch_plan_fits(g) ? (size_t)(BATCH_PLAN_HDR + batch_plan_items(g)) : 0;
}

extern "C" int ctts_batch_tile_map(const int32_t* lens, int nb0, int nb1, int M, int N, int K, int lim_m, int lim_n, int lim_k,
                                   int write_all, int32_t* tile_map, size_t map_ints, void* stream) {
  CTTS_REQUIRE(lens && tile_map && K >= 0, "ctts_batch_tile_map: bad arguments");
  const size_t need = ctts_batch_tile_map_ints(nb0, nb1, M, N);
  CTTS_REQUIRE(need > 0, "ctts_batch_tile_map: %d x %d batches of [%d, %d] do not fit a plan (ctts_batch_tile_map_ints)", nb0, nb1, M, N);
  CTTS_REQUIRE(map_ints >= need, "ctts_batch_tile_map: tile_map holds %zu int32, %zu needed", map_ints, need);
  const BatchPlanGeom g = batch_map_geom(nb0, nb1, M, N, K, lim_m, lim_n, lim_k, write_all);
  const long blocks = (batch_plan_items(g) + 255) / 256;
  hipLaunchKernelGGL(batch_tile_map_kernel, dim3((unsigned)(blocks < 64 ? blocks : 64)), dim3(256), 0, (hipStream_t)stream, g, lens, tile_map);
  CTTS_CHECK_LAUNCH("ctts_batch_tile_map");
  return 0;
}

// ---- fp32-on-bf16-pipe kernels of this file (the CALLER chooses the arithmetic, per descriptor - ctts_gemm_desc.bf16_split: 0 = fp32
// MFMA only, 1 = allowed, 2 = allowed below the size thresholds).  gemm_x6_kernel: large unbatched NT launches whose N is a multiple of
// the 128-column tile.
static bool x6_plan(const ctts_gemm_desc& d) {
  const int on = d.bf16_split;
  static const long min_tiles = ctts_env_int("CTTS_X6_MIN_TILES", 384);
  if (on < 1 || !d.a_kc || !d.b_kc || d.nb0 * d.nb1 != 1 || d.split_k > 1 || d.E || d.lens || d.conv_on_b) return false;
  if (d.K < 256 || d.K % BK || d.N % 128 || d.M < 1024) return false;
  if (d.conv_T > 0 && d.conv_cin % 4) return false;
  if (on != 2 && on != 4 && (long)((d.M + 127) / 128) * (d.N / 128) < min_tiles) return false;      // 2 / 4 = forced (tests): no size threshold
  return vec_ok(d) && buf_ok(d);
}

// the TN (weight-gradient) form: unbatched, both operands reduction-major, tile-aligned output, long reduction; CTTS_X6_TN=0 turns it off
static bool x6tn_plan(const ctts_gemm_desc& d) {
  static const int tn = ctts_env_int("CTTS_X6_TN", 1);
  static const long min_wg = ctts_env_int("CTTS_X6_TN_MIN_WG", 384);
  if (d.bf16_split < 1 || !tn || d.a_kc || d.b_kc || d.nb0 * d.nb1 != 1 || d.E || d.lens || d.epi_bwd) return false;
  if (d.M % 128 || d.N % 128 || d.K % BK || d.K < 2048) return false;
  // (a thread stages 8 consecutive reduction rows starting at a multiple of 8: they stay inside one utterance when conv_T % 8 == 0)
  if (d.conv_T > 0 && (!d.conv_on_b || d.conv_T % 8 || d.conv_cin % 4)) return false;
  if (d.bf16_split != 2 && d.bf16_split != 4 && (long)(d.M / 128) * (d.N / 128) * (d.split_k > 1 ? d.split_k : 1) < min_wg) return false;
  return vec_ok(d) && buf_ok(d);
}

static int x6tn_launch(const ctts_gemm_desc& d, hipStream_t st) {
  const dim3 grid((d.M / 128) * (d.N / 128), d.split_k > 1 ? d.split_k : 1, 1);
  if (d.conv_T > 0) hipLaunchKernelGGL(gemm_x6tn_kernel<true>, grid, dim3(256), 0, st, d);
  else hipLaunchKernelGGL(gemm_x6tn_kernel<false>, grid, dim3(256), 0, st, d);
  CTTS_CHECK_LAUNCH("ctts_gemm(x6tn)");
  return 0;
}

static int x6_launch(const ctts_gemm_desc& d, hipStream_t st) {
  const int tiles = ((d.M + 127) / 128) * (d.N / 128);
  if (d.conv_T > 0) hipLaunchKernelGGL(gemm_x6_kernel<true>, dim3(tiles), dim3(256), 0, st, d);
  else hipLaunchKernelGGL(gemm_x6_kernel<false>, dim3(tiles), dim3(256), 0, st, d);
  CTTS_CHECK_LAUNCH("ctts_gemm(x6)");
  return 0;
}

// d.tile_map of a launch with per-batch length limits is a batch tile plan (ctts_batch_tile_map), not an m-tile schedule
static bool batch_plan_given(const ctts_gemm_desc& d) {
  return d.tile_map && d.tile_map != reinterpret_cast<const int32_t*>(1) && d.lens && (d.lim_m || d.lim_n || d.lim_k);
}

// What gemm_route decides for one descriptor: the launch, the queries and the split plan all read this and nothing else.
struct GemmRoute {
  // kind; workgroup tile; split_k = K ranges that write partial matrices (the caller's, lowered until they fit; 1: none);
  // k_granule = the K granularity of a split (the kernel's `chunk`)
  ctts_gemm_route_info info;
  bool split_fits;           // false: not even two partial matrices fit (an error for a launch)
  int tile_group_n;          // descriptor adjustments of a tile-kernel launch: ctts_gemm_desc.tile_group_n ...
  bool natural_order;        // ... and the tile_map == 1 sentinel (plain blockIdx order)
  union { PlArgs pl; PlwArgs plw; WsArgs ws; SkArgs sk; };      // the planned arguments of the family that takes the launch
  GemmGrid grid;
};

// The tile-per-workgroup kernels of this file: which one, its tile, and the order it walks its tiles in.  x6tn: x6tn_plan(d).
static void tile_plan(const ctts_gemm_desc& d, bool x6tn, GemmRoute& r) {
  const long tiles128 = (long)((d.M + 127) / 128) * ((d.N + 127) / 128) * (d.split_k > 1 ? d.split_k : 1) * d.nb0 * d.nb1;
  static const int force_tile = ctts_env_int("CTTS_FORCE_TILE", 0);   // tuning knob
  static const bool natural = getenv("CTTS_NATURAL_ORDER") != nullptr;
  // XCD-grouped order for scheduled launches: default 4 n-groups (XCD x: n-group x % 4, every second scheduled m-tile) - halves the
  // L2-miss traffic of the FFN conv (FETCH_SIZE 441 -> 195 MB per launch) at unchanged time; CTTS_TILE_GROUP=<g> overrides, 0 = off.
  static const int tile_group = ctts_env_int("CTTS_TILE_GROUP", -1);
  if (tile_group != 0 && d.tile_map && d.tile_map != reinterpret_cast<const int32_t*>(1) && !batch_plan_given(d)) {
    const int tn = (d.N + 63) / 64, tmn = (d.M + 63) / 64;
    const int g = tile_group > 0 ? tile_group : ((tn >= 8 && tn % 4 == 0) ? tn / 4 : 0);
    if (g > 0 && tn % g == 0) {
      const int ng = tn / g;
      if ((ng == 1 || ng == 2 || ng == 4 || ng == 8) && tmn % (8 / ng) == 0 && ((long)tmn * tn) % 8 == 0) r.tile_group_n = g;
    }
  }
  // CTTS_TN_NATURAL: plain blockIdx order for the weight-gradient (TN, split-K) launches only.  4-12 % faster in the isolated
  // micro-benchmark (96.6 -> 86 us FFN linear, 711 -> 683 us FFN conv) - in-step effect measured separately, off by default.
  static const bool tn_natural = getenv("CTTS_TN_NATURAL") != nullptr;
  r.natural_order = (natural || (tn_natural && !d.a_kc && !d.b_kc)) && !d.tile_map;
  // 16-byte BUFFER loads only need dword-aligned addresses (the LDS side of the tile is aligned by construction), so the buffer kernels
  // also take operands whose base / leading dimension is not a multiple of 4 floats - the padded views (rows of T+1) of the relative
  // attention score slabs - as long as the chunking fits.  Pointer-based 16-byte loads (the non-buffer VEC path) need full alignment.
  const bool aligned = vec_ok(d);
#ifdef CTTS_NO_BUF
  const bool buf_unaligned = false;
#else
  const bool buf_unaligned = !aligned && chunks_ok(d) && d.conv_T <= 0 && !(d.lens && (d.lim_m || d.lim_n || d.lim_k));
#endif
  r.info.tile_m = r.info.tile_n = 64;
  if (x6tn) { r.info.kind = CTTS_GEMM_X6TN; r.info.tile_m = r.info.tile_n = 128; }      // weight gradient on the bf16-split kernel, with ordered split-K partials like the others
  else if (!aligned && !(buf_unaligned && buf_ok(d))) r.info.kind = CTTS_GEMM_SCALAR64;
#ifndef CTTS_NO_BUF
  else if (buf_ok(d)) {
    // 64x64 tiles (64 VGPRs: 8 waves/SIMD) match the 128x128 kernel on every measured shape (109 / 119 / 108 / 107 TFLOP/s on FFN conv fwd,
    // 4096^3, conv dgrad, conv wgrad) and make padded-row skipping effective: 64-row granularity and many waves per CU instead of two
    // rounds of 128-row tiles (fs2 train step 33.3 -> 29.8 ms).  CTTS_FORCE_TILE=128 keeps the big-tile kernel reachable for A/B runs.
    // under-filled forward / data-gradient launches (A K-contiguous, unbatched): few 64 x 64 tiles - the phoneme-level layers (2,048
    // rows).  Routing by the step time (same box): tile limit 160 / 320 / 640 / 1024: fs2 23.36 / 23.27 / 23.17 / 23.24 ms from 23.48,
    // conformer 27.78 / 27.84 / 27.62 / 27.90 from 28.14; K >= 256 instead of 512: another -0.03 / -0.05 ms.
    static const int k2 = ctts_env_int("CTTS_K2_TILE", 640);          // largest 64 x 64 tile count routed here (0 = off)
    static const int k2_mink = ctts_env_int("CTTS_K2_MIN_K", 256);
    // the split-K weight gradients (TN) of those layers as well: conformer 27.82 -> 27.53 ms.  NOTE: the two-group kernel has no K-block
    // skipping (row_lens / tile_map are ignored for TN launches) - correct because the rows of dZ beyond a sequence's length are exactly
    // zero (every producer of a gradient masks or zero-fills its padded rows), it merely multiplies those zeros.
    static const int k2_tn = ctts_env_int("CTTS_K2_TN", 1);
    static const bool narrow = ctts_env_int("CTTS_NARROW_TILE", 1) != 0;
    if (force_tile == 128) { r.info.kind = CTTS_GEMM_BUF128; r.info.tile_m = r.info.tile_n = 128; }
    else if (k2 && (d.a_kc || (k2_tn && !d.b_kc)) && d.nb0 * d.nb1 == 1 && !d.lens && d.N >= 64 && d.M >= 256 && d.K >= k2_mink &&
             (long)((d.M + 63) / 64) * ((d.N + 63) / 64) * (d.split_k > 1 ? d.split_k : 1) <= k2) { r.info.kind = CTTS_GEMM_BUF_K2; r.info.tile_m = 32; }
    else if (narrow && d.N <= 32 && d.M >= 256 && d.conv_T <= 0 && (!d.tile_map || batch_plan_given(d)) && !r.natural_order && !d.row_lens) { r.info.kind = CTTS_GEMM_BUF_NARROW; r.info.tile_m = 128; r.info.tile_n = 32; }
    else r.info.kind = CTTS_GEMM_BUF64;
  }
#endif
  // weight-gradient (TN) reductions measured faster on 64x64 tiles (64 VGPRs: 8 waves/SIMD): 92.6 vs 84.6 TFLOP/s on the FFN conv wgrad
  else if (tiles128 >= 256 && d.N > 64 && (d.a_kc || d.b_kc)) { r.info.kind = CTTS_GEMM_VEC128; r.info.tile_m = r.info.tile_n = 128; }
  else r.info.kind = CTTS_GEMM_VEC64;
  r.info.k_granule = r.info.kind == CTTS_GEMM_BUF_K2 ? 2 * BK : BK;
}

// THE order in which the kernel families are asked for a descriptor (nb0 / nb1 >= 1).  Pure: no launch, no error.  Tile kernels finish
// split_k > 1 as an ordered split-K (gemm_common.h; splitk_reduce_kernel above): one partial matrix [M, N] per (batch, split) - in the
// workspace, or in split_out when the caller keeps them and adds them itself later (ctts_partial_sums, many GEMMs per launch: no reduce
// launch).  split_k is an upper bound, lowered until the partials fit (never below 2 - "C += alpha A B" is what split_k > 1 means);
// unbounded_room: the split plan, whose caller sizes split_out from the answer.
static void gemm_route(const ctts_gemm_desc& d, GemmRoute& r, bool unbounded_room = false) {
  r.info = ctts_gemm_route_info{CTTS_GEMM_NONE, 128, 128, 1, 32};
  r.split_fits = true;
  r.tile_group_n = 0;
  r.natural_order = false;
  bool x6tn = false;
  if (ctts_gemm_pl_plan(d, r.pl, r.grid)) r.info.kind = CTTS_GEMM_PLANES;                  // pre-split bf16 planes given and eligible: persistent plane kernel
  else if (ctts_gemm_plw_plan(d, r.plw, r.grid)) r.info.kind = CTTS_GEMM_PLANES_WGRAD;     // ... in the weight-gradient layout: adds into C itself, no partial matrices
  else if (ctts_gemm_ws_plan(d, r.ws, r.grid)) r.info.kind = CTTS_GEMM_WEIGHT_STATIONARY;  // K = 256 linears with many rows
  else if (x6_plan(d)) { r.info.kind = CTTS_GEMM_X6; return; }                             // fp32 products on the bf16 matrix pipe (six-term split), 128 x 128 tiles
  else if (!(x6tn = x6tn_plan(d)) && ctts_gemm_sk_plan(d, r.sk, r.grid)) r.info.kind = CTTS_GEMM_STREAM_K;      // (x6's weight-gradient form goes before stream-K)
  if (r.info.kind != CTTS_GEMM_NONE) { r.info.tile_m = r.grid.tile_m; r.info.tile_n = r.grid.tile_n; return; }
  tile_plan(d, x6tn, r);
  if (d.split_k > 1) {
    const long per_split = (long)d.nb0 * d.nb1 * d.M * gemm_partial_ld(d.N);
    const long room = unbounded_room ? (1L << 60) : (d.split_out ? d.split_out_floats : (long)CTTS_WS_SLAB_FLOATS);
    const long cap = per_split > 0 ? room / per_split : 0;
    r.split_fits = cap >= 2 && (long)d.M * gemm_partial_ld(d.N) * 4 < 0x7FFF0000L;
    r.info.split_k = d.split_k > cap ? (int)cap : d.split_k;
  }
}

// what ctts_gemm checks before it routes: 0 = go on with `d` (normalised copy), 1 = nothing to do (empty output), < 0 = error
static int gemm_validate(const ctts_gemm_desc* dp, ctts_gemm_desc& d) {
  CTTS_REQUIRE(dp != nullptr, "ctts_gemm: null descriptor");
  d = gemm_normalized(*dp);
  CTTS_REQUIRE(d.A && d.B && d.C, "ctts_gemm: null operand pointer");
  CTTS_REQUIRE(d.M >= 0 && d.N >= 0 && d.K >= 0, "ctts_gemm: negative dimension");
  if (d.M == 0 || d.N == 0) return 1;
  if (d.conv_T > 0) {
    CTTS_REQUIRE(d.conv_cin > 0 && (d.conv_cin % 4) == 0, "ctts_gemm: conv view needs cin %% 4 == 0 (got %d)", d.conv_cin);
    CTTS_REQUIRE(d.conv_on_b ? (!d.a_kc && !d.b_kc) : (d.a_kc != 0), "ctts_gemm: conv view on an unsupported operand layout");
  }
  CTTS_REQUIRE(d.p_drop >= 0.f && d.p_drop < 1.f, "ctts_gemm: p_drop out of range");
  CTTS_REQUIRE(!d.epi_bwd || (d.split_k <= 1 && !d.bias && !d.R && !d.rowscale && !d.E && (!d.act || d.Z)),
               "ctts_gemm: epi_bwd excludes bias, residual, rowscale, E and split-K, and needs Z when an activation is given");
  CTTS_REQUIRE(!d.E || (d.rowsub && d.split_k <= 1 && !d.bias && !d.act && d.p_drop == 0.f && !d.R && !d.rowscale && !d.Z),
               "ctts_gemm: the E/rowsub epilogue excludes bias, activation, dropout, residual, rowscale and split-K");
  CTTS_REQUIRE(!batch_plan_given(d) || (!d.row_lens && d.split_k <= 1 && batch_plan_fits(batch_plan_geom(d, 64, 64, 1))),
               "ctts_gemm: a batch tile plan (tile_map on a launch with length limits) excludes row_lens and split-K, and the batches "
               "must fit one (ctts_batch_tile_map_ints)");
  return 0;
}

// validate -> route -> a tile-kernel launch with split_k > 1 needs somewhere to put its partial matrices.  Returns like gemm_validate.
static int gemm_plan(const ctts_gemm_desc* dp, ctts_gemm_desc& d, GemmRoute& r) {
  const int rc = gemm_validate(dp, d);
  if (rc != 0) return rc;
  gemm_route(d, r);
  // only the 64 x 64 buffer kernel with per-batch limits follows a batch tile plan: on any other route the map would be read as an
  // m-tile schedule, or not at all
  CTTS_REQUIRE(!batch_plan_given(d) || r.info.kind == CTTS_GEMM_BUF64,
               "ctts_gemm: a batch tile plan was given, but the launch does not run on the 64 x 64 buffer kernel (route kind %d)", r.info.kind);
  if (r.info.kind < CTTS_GEMM_X6TN || d.split_k <= 1) return 0;
  CTTS_REQUIRE(d.split_out || (d.sk_ws && d.sk_ws_bytes >= (int64_t)CTTS_WS_BYTES),
               "ctts_gemm: split_k > 1 needs the workspace (ctts_workspace_bytes() bytes, zero-filled once) in sk_ws - partial sums "
               "are added in a fixed order through it, the library has no floating-point atomics");
  CTTS_REQUIRE(r.split_fits, "ctts_gemm: split-K output [%d, %d] x %d batches does not fit the %s", d.M, d.N, d.nb0 * d.nb1,
               d.split_out ? "caller's split_out buffer" : "workspace");
  return 0;
}

extern "C" int ctts_gemm(const ctts_gemm_desc* dp, void* stream) {
  ctts_gemm_desc d;
  GemmRoute r;
  int rc = gemm_plan(dp, d, r);
  if (rc != 0) return rc < 0 ? rc : 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // ---- `t` is the descriptor the tile kernels see (the other families take the caller's)
  const bool split = r.info.split_k > 1;
  ctts_gemm_desc t = d;
  t.tile_group_n = r.tile_group_n;
  if (r.natural_order) t.tile_map = reinterpret_cast<const int32_t*>(1);
  if (d.split_k > 1) t.split_k = r.info.split_k;      // (possibly lowered)
  const ctts_gemm_desc d_user = t;                 // what the reduce launch accumulates into
  if (split) {
    // the tile kernels see the partial matrices as their output: C = P [z][split][M][ldp], plain stores (alpha = 1, no epilogue terms);
    // workgroup (z, split) adds split * M * ldc itself.  Whole tiles of padded rows are "zero-filled" into P_0 and skipped by the reduce.
    const long ldp = gemm_partial_ld(d.N);
    t.C = d.split_out ? d.split_out : reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(d.sk_ws) + CTTS_WS_SLABS);
    t.ldc = ldp;
    t.sC1 = (long)t.split_k * d.M * ldp;
    t.sC0 = (long)d.nb1 * t.sC1;
    t.alpha = 1.f; t.bias = nullptr; t.Z = nullptr; t.act = 0; t.p_drop = 0.f; t.R = nullptr; t.rowscale = nullptr;
  }
  switch (r.info.kind) {
    case CTTS_GEMM_PLANES: return ctts_gemm_pl_launch(d, r.pl, r.grid, st);
    case CTTS_GEMM_PLANES_WGRAD: return ctts_gemm_plw_launch(d, r.plw, r.grid, st);
    case CTTS_GEMM_WEIGHT_STATIONARY: return ctts_gemm_ws_launch(d, r.ws, r.grid, st);
    case CTTS_GEMM_X6: return x6_launch(d, st);
    case CTTS_GEMM_STREAM_K: return ctts_gemm_sk_launch(d, r.sk, r.grid, st);
    case CTTS_GEMM_SCALAR64: rc = for_layout<true>(t, [&](auto a, auto b, auto c) { return launch_tile<64, 64, a(), b(), c(), Fetch::Scalar>(t, st); }); break;
#ifndef CTTS_NO_BUF
    case CTTS_GEMM_BUF128: rc = for_layout<true>(t, [&](auto a, auto b, auto c) { return launch_tile<128, 128, a(), b(), c(), Fetch::Buffer>(t, st); }); break;
    case CTTS_GEMM_BUF_K2: rc = for_layout<true>(t, [&](auto a, auto b, auto c) { return launch_buf_k2<a(), b(), c()>(t, st); }); break;
    // 128 x 32 tiles (4 x 1 waves) for outputs at most 32 columns wide: with 64 x 64 tiles half of every workgroup's MFMAs would multiply
    // zero columns.  The three products of the conformer's attention backward that consume dS ([T, 32] = [T, T] x [T, 32] per (b, h),
    // ctts_relmha_bwd) are the users.  No conv views.
    case CTTS_GEMM_BUF_NARROW: rc = for_layout<false>(t, [&](auto a, auto b, auto c) { return launch_tile<128, 32, a(), b(), c(), Fetch::Buffer>(t, st); }); break;
    case CTTS_GEMM_BUF64: rc = for_layout<true>(t, [&](auto a, auto b, auto c) { return launch_tile<64, 64, a(), b(), c(), Fetch::Buffer>(t, st); }); break;
#endif
    case CTTS_GEMM_VEC128: rc = for_layout<true>(t, [&](auto a, auto b, auto c) { return launch_tile<128, 128, a(), b(), c(), Fetch::Vec>(t, st); }); break;
    case CTTS_GEMM_X6TN: rc = x6tn_launch(t, st); break;
    default: rc = for_layout<true>(t, [&](auto a, auto b, auto c) { return launch_tile<64, 64, a(), b(), c(), Fetch::Vec>(t, st); }); break;
  }
  if (rc != 0 || !split || d.split_out) return rc;
  return splitk_reduce(d_user, r.info.tile_m, r.info.k_granule, st);
}

extern "C" int ctts_gemm_route(const ctts_gemm_desc* dp, ctts_gemm_route_info* info) {
  CTTS_REQUIRE(info != nullptr, "ctts_gemm_route: null info");
  *info = ctts_gemm_route_info{CTTS_GEMM_NONE, 0, 0, 0, 0};
  ctts_gemm_desc d;
  GemmRoute r;
  const int rc = gemm_plan(dp, d, r);
  if (rc == 0) *info = r.info;
  return rc < 0 ? rc : 0;
}

static int route_kind(const ctts_gemm_desc* dp) {          // of an unvalidated descriptor
  if (!dp) return CTTS_GEMM_NONE;
  const ctts_gemm_desc d = gemm_normalized(*dp);
  GemmRoute r;
  gemm_route(d, r);
  return r.info.kind;
}
extern "C" int ctts_gemm_takes_planes(const ctts_gemm_desc* d) {
  const int kind = route_kind(d);
  return kind == CTTS_GEMM_PLANES || kind == CTTS_GEMM_PLANES_WGRAD;
}
extern "C" int ctts_gemm_takes_bf16_split(const ctts_gemm_desc* d) {
  const int kind = route_kind(d);
  return kind == CTTS_GEMM_X6 || kind == CTTS_GEMM_X6TN;
}

// Deferred split-K (ctts_gemm_desc.split_out): would ctts_gemm run this descriptor as a split-K launch of the tile kernels whose partial
// matrices the caller may keep and add later?  Returns 1 and fills *count (partial matrices that will be written: P_0 .. P_count-1) and
// *stride (floats between them; each is [M, N rounded up to 4] row-major), else 0 (another family takes it, split_k <= 1, batched or
// length-limited launches).  Give ctts_gemm a split_out buffer of at least split_k * stride floats.
extern "C" int ctts_gemm_split_plan(const ctts_gemm_desc* dp, int32_t* count, int64_t* stride) {
  ctts_gemm_desc d;
  GemmRoute r;
  if (gemm_validate(dp, d) != 0 || d.split_k <= 1) return 0;
  d.split_out = nullptr;
  // The plane forward kernel (NT) takes split_k > 1 with split_overwrite as a plain overwrite and writes no partials, yet this query
  // has always answered for an NT descriptor as if no planes were given (include/ctts.h says so); no caller defers an NT launch.
  if (d.a_kc) d.A_planes = nullptr;
  gemm_route(d, r, true);
  if (r.info.kind < CTTS_GEMM_X6TN || !r.split_fits) return 0;
  if (d.nb0 * d.nb1 != 1 || d.lens || d.K <= 0 || (d.a_kc && d.row_lens)) return 0;
  if (count) *count = gemm_split_range(d.K, r.info.split_k, r.info.k_granule, 0).nonempty;
  if (stride) *stride = (long)d.M * gemm_partial_ld(d.N);
  return 1;
}
