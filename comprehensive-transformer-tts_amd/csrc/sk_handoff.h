// Device side of the stream-K work partition (sk_plan.h), shared by the three persistent kernels gemm_sk_kernel (gemm_sk.hip),
// gemm_pl_kernel (gemm_pl.hip) and gemm_plw_kernel (gemm_plw.hip): the raw-buffer descriptor and the LDS-DMA instruction of their
// loaders, the limits of the workspace header, and THE fixed-order hand-off of a cut tile (sk_slab_publish / sk_slab_collect) - the one
// place where the protocol that decides determinism, and that hangs a GPU when it is wrong, is defined.  gemm_sk_kernel and
// gemm_plw_kernel call the two functions; gemm_pl_kernel carries the same text written out (calling them measured 0.3 - 1 % slower there,
// see the comment in gemm_pl.hip): a change here is a change there.
// Device code only: sk_plan.h stays free of it (tests/test_sk_plan_cpu.py compiles that header with g++).
#pragma once
#include "ctts_common.h"
#include "gemm_common.h"
#include "sk_plan.h"

namespace {

typedef unsigned int sk_u32x4 __attribute__((ext_vector_type(4)));
typedef int sk_i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned int sk_gu32;

// header of the workspace: flags[0 .. SK_MAX_WG - 1], one per workgroup of the grid, and the error word at [SK_MAX_WG]
constexpr int SK_MAX_WG = 2048;
constexpr int SK_SLAB_FLOATS_MAX = 2048 * 4096;      // slab area: grid x (tile rows x tile columns) floats never exceeds this (host check)
static_assert((size_t)SK_SLAB_FLOATS_MAX <= CTTS_WS_SLAB_FLOATS, "stream-K slabs exceed the workspace slab area");

// raw buffer descriptor (2 GiB window, 32-bit raw-buffer format) as four SGPR words for the inline-asm DMA below
__device__ __forceinline__ sk_i32x4 sk_make_rsrc(const void* base) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  sk_i32x4 r;
  r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
  r.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
  r.z = 0x7FFFFFFE;
  r.w = 0x00020000;
  return r;
}

// One LDS-DMA instruction: 64 lanes x 16 bytes, global (descriptor + voff + soff) -> LDS [lds_addr + lane * 16).  Inline asm on purpose:
// hipcc's waitcnt pass knows nothing about it, so it does not put `s_waitcnt vmcnt(0)` in front of every ds_read that follows (it does
// for the builtin, because it cannot prove that the DMA target and the fragment reads are different LDS stages), and the loop's own
// `s_waitcnt vmcnt(N)` + `s_barrier` stay the only synchronisation between the DMA and its readers.
__device__ __forceinline__ void sk_dma16(sk_i32x4 rsrc, unsigned lds_addr, unsigned voff, unsigned soff) {
  asm volatile("s_mov_b32 m0, %0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :: "s"(__builtin_amdgcn_readfirstlane(lds_addr)), "v"(voff), "s"(rsrc), "s"(__builtin_amdgcn_readfirstlane(soff))
               : "memory");      // m0 is not on the clobber list (hipcc rejects reserved registers there); nothing else in the kernels
                                 // that use this uses m0 - check the ISA (grep m0) when adding LDS-direct / GWS / movrel code
}

// the shared slab area of the workspace (ctts_common.h) as a buffer resource; slab of workgroup b at b * SLAB floats
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sk_slab_rsrc(unsigned* ws) {
  float* slabs = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(ws) + CTTS_WS_SLABS);
  return __builtin_amdgcn_make_buffer_rsrc((void*)slabs, 0, 0x7FFFFFFE, 0x00020000);
}

// ---- The hand-off of a cut tile.  A workgroup of WAVES waves, each with MT x NT accumulators of a 32 x 32 MFMA tile, owns a slab of
//      WAVES * MT * NT * 1024 floats: wave w's share starts at w * MT * NT * 1024, MFMA tile (i, j) = tile t = i * NT + j of the wave
//      and register quad q of it form element n = 4 t + q - 1024 floats, lane L at + 4 L (one 16-byte access per lane and element).

// A contribution (a piece with kb_hi < nkb): the accumulator goes to this workgroup's slab with write-through stores, the stores are
// drained, every wave has arrived, THEN the flag is raised.
template <int MT, int NT, int WAVES>
__device__ __forceinline__ void sk_slab_publish(const floatx16 (&acc)[MT][NT], __amdgpu_buffer_rsrc_t rs_src, unsigned* flags, int wave,
                                                int lane, int tid) {
  constexpr int SLAB = WAVES * MT * NT * 1024;
  const unsigned base = (unsigned)blockIdx.x * (SLAB * 4) + (unsigned)(wave * (SLAB / WAVES) + lane * 4) * 4u;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sk_u32x4 v;
        v.x = __float_as_uint(acc[i][j][4 * q + 0]); v.y = __float_as_uint(acc[i][j][4 * q + 1]);
        v.z = __float_as_uint(acc[i][j][4 * q + 2]); v.w = __float_as_uint(acc[i][j][4 * q + 3]);
        __builtin_amdgcn_raw_buffer_store_b128(v, rs_src, base + (unsigned)(((i * NT + j) * 4 + q) * 1024), 0, 16);      // aux 16 = sc1
      }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) __hip_atomic_store((sk_gu32*)(flags + blockIdx.x), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The owner of a cut tile (the piece `cp` with kb_lo > 0 and kb_hi == nkb of workgroup wj of XCD xcd): add the slabs of the workgroups
// below, nearest first, until the tile's unit 0 is covered.  Every accumulator element receives the slabs in that one order, whatever
// the timing: the sum is deterministic for a given grid.  The wait is bounded (the error word reports instead of hanging), the flag is
// cleared by its reader (the workspace is clean for the next launch).
// BATCH 16-byte loads of a slab are in flight, THEN their sums: written as "load, add" hipcc reused one register quad and waited for
// every load - MT * NT * 4 dependent L2 round trips (~1 us each) per slab on the critical path of every cut tile.
template <int MT, int NT, int WAVES, int BATCH>
__device__ __forceinline__ void sk_slab_collect(floatx16 (&acc)[MT][NT], __amdgpu_buffer_rsrc_t rs_src, unsigned* flags, const SkGeom& g,
                                                const SkRange& rg, const SkPiece& cp, int nkb, int xcd, int wj, int wave, int lane, int tid) {
  constexpr int SLAB = WAVES * MT * NT * 1024;
  static_assert((MT * NT * 4) % BATCH == 0, "a batch is a whole number of quads of the wave's share");
  const int tile_lo = cp.t * nkb;
  const int Ux = (rg.T1 - rg.T0) * nkb;
  int upper = rg.lo;                                   // start of the range that is already summed
  for (int jj = wj - 1; jj >= 0 && upper > tile_lo; --jj) {
    const int blo = sk_bound(g, Ux, jj);
    if (blo >= upper) continue;                        // empty range: that workgroup published nothing
    upper = blo;
    const int src = jj * 8 + xcd;
    if (tid == 0) {
      unsigned spins = 0;
      while (__hip_atomic_load((sk_gu32*)(flags + src), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 1u) {
        __builtin_amdgcn_s_sleep(8);
        if (++spins > (1u << 24)) {                    // bounded: report instead of hanging
          __hip_atomic_store((sk_gu32*)(flags + SK_MAX_WG), 1u + (unsigned)src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
      __hip_atomic_store((sk_gu32*)(flags + src), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // self-cleaning
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned base = (unsigned)src * (SLAB * 4) + (unsigned)(wave * (SLAB / WAVES) + lane * 4) * 4u;
#pragma unroll
    for (int b = 0; b < MT * NT * 4 / BATCH; ++b) {
      sk_u32x4 sv[BATCH];
#pragma unroll
      for (int e = 0; e < BATCH; ++e) sv[e] = __builtin_amdgcn_raw_buffer_load_b128(rs_src, base + (unsigned)((b * BATCH + e) * 1024), 0, 0);
#pragma unroll
      for (int e = 0; e < BATCH; ++e) {
        const int n = b * BATCH + e, i = (n >> 2) / NT, j = (n >> 2) % NT, q = n & 3;
        acc[i][j][4 * q + 0] += __uint_as_float(sv[e].x); acc[i][j][4 * q + 1] += __uint_as_float(sv[e].y);
        acc[i][j][4 * q + 2] += __uint_as_float(sv[e].z); acc[i][j][4 * q + 3] += __uint_as_float(sv[e].w);
      }
    }
  }
}

}  // namespace
