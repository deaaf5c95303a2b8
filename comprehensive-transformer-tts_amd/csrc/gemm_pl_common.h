// Shared pieces of the plane kernels (gemm_pl.hip: forward / data-gradient layout; gemm_plw.hip: weight-gradient layout): the bf16 MFMA,
// the fragment registers and the six-term product of a k-step, sizes of the 128 x 256 tile, the laundering in front of the epilogue and
// the host-side launch.  The loaders' buffer descriptor and LDS-DMA instruction, the workspace limits and the slab hand-off of a cut
// tile are those of all three stream-K kernels: sk_handoff.h.
#pragma once
#include "ctts_common.h"
#include "gemm_common.h"
#include "sk_handoff.h"

namespace {

typedef __bf16 pl_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 pl_bf16x2 __attribute__((ext_vector_type(2)));
typedef float pl_floatx2 __attribute__((ext_vector_type(2)));

// CTTS_PL_DEBUG bits (tools builds only: -DCTTS_PL_TOOLS; the product build compiles them out - their scalar branches and the clock
// stamps cost the conv instantiation three spilled VGPRs with reloads inside the K loop)
#ifdef CTTS_PL_TOOLS
#define PL_DBG(bit) (p.debug & (bit))
#else
#define PL_DBG(bit) 0
#endif

constexpr unsigned PL_OOB = 0x80000000u;
constexpr int PL_BM = 128, PL_BN = 256;
constexpr int PL_ROW = 64;                                    // bytes per plane row of a 32-deep K-block
constexpr int PL_A_PLANE = PL_BM * PL_ROW, PL_B_PLANE = PL_BN * PL_ROW;
constexpr int PL_STAGE = 3 * (PL_A_PLANE + PL_B_PLANE);       // 73,728 bytes
constexpr int PL_SLAB = PL_BM * PL_BN;                        // floats per workgroup slab (8 waves x 2 x 2 MFMA tiles: sk_handoff.h)
constexpr int PL_MAX_UTT = 256;


__device__ __forceinline__ floatx16 pl_mma(const sk_u32x4 a, const sk_u32x4 b, const floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(pl_bf16x8, a), __builtin_bit_cast(pl_bf16x8, b), c, 0, 0, 0);
}

struct PlFrag { sk_u32x4 a[2][3], b[2][3]; };      // one 16-deep k-step: [MFMA row / column tile][piece]

__device__ __forceinline__ void pl_zero_acc(floatx16 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// terms [t0, t1) of the six-term product of one k-step; term-major: consecutive MFMAs hit different accumulators; smallest terms first.
// TERMS = 6: fp32 products from the six cross terms of the three-way split (bf16_split 1 / 2).  TERMS = 1: the "amp" arithmetic
// (bf16_split 3 / 4; reference train.py:59,104 `amp.autocast`): operands ROUNDED to bf16 - only the hi pieces are moved and multiplied -
// fp32 accumulate: one MFMA term, a third of the operand traffic.  Never the default, reported separately.
template <int TERMS>
__device__ __forceinline__ void pl_mma_terms(floatx16 (&acc)[2][2], const PlFrag& f, int t0, int t1) {
  if constexpr (TERMS == 1) {          // hi x hi only
    if (t0 <= 5 && 5 < t1) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = pl_mma(f.a[i][0], f.b[j][0], acc[i][j]);
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
    if (t < t0 || t >= t1) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = pl_mma(f.a[i][PA[t]], f.b[j][PB[t]], acc[i][j]);
  }
}

// "The piece is complete": what runs behind the K loop once per piece must not cost the loop registers.  (1) The lane / wave constants
// l31, h, wm0, wn0 of the enclosing kernel are laundered through an empty asm (-> e_l31, e_h, e_wm0, e_wn0) so that loop-invariant code
// motion cannot hoist the epilogues' lane offsets in front of the K loop.  (2) The descriptor fields only the epilogue needs (C, Z, bias,
// strides, dropout, ...) are read from the kernel-argument segment (the descriptor is the first kernel argument: offset 0) through a
// laundered pointer (-> dc): s_load at the point of use instead of ~60 SGPRs that stay live across the K loop - hipcc preloads a
// by-value struct argument and then spills it to VGPR lanes (560 SGPR spills, 27 VGPR spills and scratch reloads in front of every DMA
// issue in the first build of gemm_pl_kernel).
#define PL_PIECE_COMPLETE()                                                                                                   \
  int e_l31 = l31, e_h = h, e_wm0 = wm0, e_wn0 = wn0;                                                                         \
  unsigned long long kargs_ = (unsigned long long)(const void*)__builtin_amdgcn_kernarg_segment_ptr();                        \
  asm volatile("" : "+v"(e_l31), "+v"(e_h), "+s"(e_wm0), "+s"(e_wn0), "+s"(kargs_));                                          \
  const ctts_gemm_desc& dc = *(const ctts_gemm_desc*)(const __attribute__((address_space(4))) ctts_gemm_desc*)kargs_

// host side: a plane kernel has four instantiations - conv view on / off x one MFMA term (the "amp" arithmetic, bf16_split 3 / 4) or six
template <class Kern, class Args>
int pl_launch(Kern conv_1, Kern dense_1, Kern conv_6, Kern dense_6, const ctts_gemm_desc& d, const Args& p, int grid, hipStream_t st, const char* what) {
  const Kern k = d.bf16_split >= 3 ? (d.conv_T > 0 ? conv_1 : dense_1) : (d.conv_T > 0 ? conv_6 : dense_6);
  hipLaunchKernelGGL(k, dim3(grid), dim3(512), 0, st, d, p);
  CTTS_CHECK_LAUNCH(what);
  return 0;
}

}  // namespace
