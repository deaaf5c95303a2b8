// HiFi-GAN V1 generator, half-precision (fp16) inference mode: the layers of csrc/vocoder.hip with fp16 weights and activations on
// v_mfma_f32_32x32x16_f16, one MFMA term per product (include/ctts.h, "fp16 mode" - the arithmetic contract lives there).
// The layer geometry, the epilogue walk and conv_post (vpost_kernel<_Float16>) are vocoder_common.h's.
// Accepted, V1 or not: B, T, Cin, Cout >= 1; Conv1d with odd k and (k - 1) dil <= 64; ConvTranspose1d with k % u == 0, (k - u) even and
// k / u <= 65; fp16 or fp32 input of any strides (tests/test_vocoder_contract_gpu.py runs the edges of this contract).
//
// vconv_h_kernel: the implicit GEMM of vconv_kernel (rows = positions of one utterance, N = output columns, K = taps x Cin; on-load
//   leaky_relu; out = fp16(beta * out + alpha * (acc + bias + R))) reshaped for one operand plane:
//   - a workgroup owns BM = 128 positions x BN columns.  A 256-row instantiation (a staged weight block serves twice the positions:
//     16 MFMAs per wave and tap from 12 ds_read_b128 at BN = 128) exists behind CTTS_VOCODER_H_BM=256 and measured SLOWER (DESIGN.md
//     section 8): 190 VGPRs leave two waves per SIMD where the 128-row tile keeps four.  The tile height does not change a single bit:
//     an output element is one lane's accumulator over a K order (32-channel chunk, tap, channel) that no tile shape enters.
//   - the weight K-block (BN x 32 fp16 = 8 KB at BN = 128) is double-buffered in LDS: the next tap's block is fetched into registers
//     before the current tap's MFMAs, stored into the other buffer after them, and ONE barrier per tap orders both (vconv_kernel: two).
//   - LDS per workgroup: (BM + 64) x 64 B input rows + 2 x BN x 64 B weights = 36 KB at 256 x 128, 28 KB at 128 x 128.
//   Input rows are 64 bytes (32 fp16 of one chunk), the four 16-byte pieces XOR-swizzled by (row >> 2) & 3 - the single-plane image of
//   vconv_kernel's split tiles, read by the same ds_read_b128 pattern.
#include "vocoder_common.h"
#include <stdlib.h>

namespace {

typedef _Float16 vh_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int vh_u32x4 __attribute__((ext_vector_type(4)));

constexpr float VH_MAX = 65504.f;          // largest finite fp16

struct VhParams {
  VcGeom g;
  const void* x; long sxb, sxt, sxc; int x_f32, vec;
  const uint16_t* w; const _Float16* R; _Float16* out;
};

// the one rounding of a stored value: saturate to +-65504, then round to nearest even (NaN stays NaN)
__device__ __forceinline__ _Float16 vh_round(float v) {
  v = v > VH_MAX ? VH_MAX : (v < -VH_MAX ? -VH_MAX : v);
  return (_Float16)v;
}

__device__ __forceinline__ int vh_sw(int row, int c) { return c ^ ((row >> 2) & 3); }

template <int BM, int BN>
__global__ __launch_bounds__(256, 2) void vconv_h_kernel(const VhParams p) {
  constexpr int NT = BN == 128 ? 2 : 1;
  constexpr int WAVES_N = BN / (32 * NT);             // 2, 2, 1
  constexpr int WAVES_M = 4 / WAVES_N;                // 2, 2, 4
  constexpr int MT = BM / (32 * WAVES_M);             // BM = 256: 4, 4, 2;  128: 2, 2, 1
  constexpr int AROWS = BM + VC_HALO_MAX;
  constexpr int B_BYTES = BN * 64;                    // one staged weight K-block
  constexpr int B_CHUNKS = BN * 4;                    // its 16-byte pieces
  constexpr int B_PER_T = (B_CHUNKS + 255) / 256;
  __shared__ __attribute__((aligned(16))) unsigned char smem[AROWS * 64 + 2 * B_BYTES];
  unsigned char* sA = smem;
  unsigned char* sB = smem + AROWS * 64;

  const VcGeom& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, m0 = blockIdx.x * BM, col0 = blockIdx.y * BN;
  const int wm0 = (wave / WAVES_N) * (MT * 32), wn0 = (wave % WAVES_N) * (NT * 32);
  // ragged (include/ctts.h): the utterance's own length replaces T everywhere below; a tile at or beyond its end has nothing to do
  const int Tb = vc_rows(g.lens, b, g.len_mul, g.T), Mb = Tb + g.mextra, Toutb = g.u ? Tb * g.u : Tb;
  if (Tb == 0 || m0 >= Mb) return;
  const int p0 = g.row_off + m0;                      // position of tile row 0
  const int nchunks = g.cin_pad >> 5, taps = g.taps;
  const long kp = (long)taps * g.cin_pad;             // packed weight row length (fp16 elements)
  const int arows = BM + (taps - 1) * g.dil;

  vc_floatx16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  vh_u32x4 rb[B_PER_T];
  // weight K-block kbg (= tap * nchunks + chunk) of columns col0 .. col0 + BN into registers (the packed rows are padded to 128 columns)
  auto load_b = [&](int kbg) {
#pragma unroll
    for (int i = 0; i < B_PER_T; ++i) {
      const int idx = tid + 256 * i;
      if (B_CHUNKS % 256 == 0 || idx < B_CHUNKS) {
        const int n = idx >> 2, c = idx & 3;
        rb[i] = *reinterpret_cast<const vh_u32x4*>(p.w + (long)(col0 + n) * kp + (long)kbg * 32 + c * 8);
      }
    }
  };
  auto store_b = [&](int buf) {
#pragma unroll
    for (int i = 0; i < B_PER_T; ++i) {
      const int idx = tid + 256 * i;
      if (B_CHUNKS % 256 == 0 || idx < B_CHUNKS) {
        const int n = idx >> 2, c = idx & 3;
        *reinterpret_cast<vh_u32x4*>(sB + buf * B_BYTES + n * 64 + vh_sw(n, c) * 16) = rb[i];
      }
    }
  };
  // input rows p0 + in_off + i (i < arows), channels chunk * 32 .. + 31 as fp16(leaky_relu(float(x))), zero outside [0, Tb) x [0, Cin)
  auto stage_a = [&](int chunk) {
    const int c8 = tid & 3, cbase = chunk * 32 + c8 * 8;
    for (int i = tid >> 2; i < arows; i += 64) {
      const int ti = p0 + g.in_off + i;
      vh_f16x8 hv;
#pragma unroll
      for (int e = 0; e < 8; ++e) hv[e] = (_Float16)0.f;
      if (ti >= 0 && ti < Tb) {
        const long roff = (long)b * p.sxb + (long)ti * p.sxt;
        if (p.vec) {
          if (cbase < g.Cin) hv = *reinterpret_cast<const vh_f16x8*>(reinterpret_cast<const _Float16*>(p.x) + roff + cbase);   // act_in = 0: taken as it is - no rounding, so no saturation (include/ctts.h)
          if (g.act_in) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float v = (float)hv[e];
              hv[e] = vh_round(v > 0.f ? v : v * g.slope);
            }
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (cbase + e < g.Cin) {
              const long off = roff + (long)(cbase + e) * p.sxc;
              float v = p.x_f32 ? reinterpret_cast<const float*>(p.x)[off] : (float)reinterpret_cast<const _Float16*>(p.x)[off];
              if (g.act_in) v = v > 0.f ? v : v * g.slope;
              hv[e] = vh_round(v);
            }
        }
      }
      *reinterpret_cast<vh_f16x8*>(sA + i * 64 + vh_sw(i, c8) * 16) = hv;
    }
  };
  // lane (l31, h) supplies k = 16 ks + 8 h + 0..7 of the 32-deep block to MFMA step ks (the same map for A and B)
  auto compute = [&](int shift, int buf) {
    vh_f16x8 fa[2][MT], fb[2][NT];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int row = wm0 + i * 32 + l31 + shift;
        fa[ks][i] = *reinterpret_cast<const vh_f16x8*>(sA + row * 64 + vh_sw(row, ks * 2 + h) * 16);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int row = wn0 + j * 32 + l31;
        fb[ks][j] = *reinterpret_cast<const vh_f16x8*>(sB + buf * B_BYTES + row * 64 + vh_sw(row, ks * 2 + h) * 16);
      }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ks][i], fb[ks][j], acc[i][j], 0, 0, 0);
  };

  load_b(0);
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    __syncthreads();                       // every wave is done with the previous chunk's input tile and weight buffers
    stage_a(chunk);
    store_b(0);
    __syncthreads();
    for (int tap = 0; tap < taps; ++tap) {
      if (tap + 1 < taps) load_b((tap + 1) * nchunks + chunk);
      else if (chunk + 1 < nchunks) load_b(chunk + 1);
      compute(tap * g.dil, tap & 1);
      if (tap + 1 < taps) {
        store_b((tap + 1) & 1);            // the buffer tap - 1 was read from: every wave left that read before the previous barrier
        __syncthreads();
      }
    }
  }

  vc_epilogue<MT, NT>(g, acc, b, m0, col0, wm0, wn0, l31, h, Mb, Toutb,
                      [R = p.R, out = p.out, alpha = g.alpha, beta = g.beta](long idx, float v) {
    if (R) v += (float)R[idx];
    v *= alpha;
    if (beta != 0.f) v = beta * (float)out[idx] + v;
    out[idx] = vh_round(v);
  });
}

template <int BM>
void vconv_h_launch(const VhParams& p, int BN, int B, hipStream_t st) {
  const dim3 grid = vc_grid(p.g, BM, BN, B);
  if (BN == 128) hipLaunchKernelGGL((vconv_h_kernel<BM, 128>), grid, dim3(256), 0, st, p);
  else if (BN == 64) hipLaunchKernelGGL((vconv_h_kernel<BM, 64>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((vconv_h_kernel<BM, 32>), grid, dim3(256), 0, st, p);
}

}  // namespace

extern "C" int ctts_vocoder_conv_h(const ctts_vconv_h_desc* dp, void* stream) {
  CTTS_REQUIRE(dp, "ctts_vocoder_conv_h: NULL descriptor");
  const ctts_vconv_h_desc& d = *dp;
  CTTS_REQUIRE(d.x && d.w && d.out, "ctts_vocoder_conv_h: x, w and out are required");
  VhParams p{};
  int BN;
  if (int rc = vc_geometry("ctts_vocoder_conv_h", d.B, d.T, d.Cin, d.Cout, d.k, d.dil, d.transposed_u, d.lens, d.len_mul, p.g, BN)) return rc;
  p.g.act_in = d.act_in; p.g.slope = d.slope; p.g.alpha = d.alpha; p.g.beta = d.beta; p.g.bias = d.bias;
  p.x = d.x; p.sxb = d.sxb; p.sxt = d.sxt; p.sxc = d.sxc; p.x_f32 = d.x_f32 != 0;
  p.w = d.w; p.R = reinterpret_cast<const _Float16*>(d.R); p.out = reinterpret_cast<_Float16*>(d.out);
  CTTS_REQUIRE(((uintptr_t)d.w & 15) == 0, "ctts_vocoder_conv_h: packed weights must be 16-byte aligned");
  CTTS_REQUIRE(((uintptr_t)d.out & 1) == 0 && ((uintptr_t)d.R & 1) == 0 && ((uintptr_t)d.x & (p.x_f32 ? 3 : 1)) == 0,
               "ctts_vocoder_conv_h: misaligned x, R or out");
  CTTS_REQUIRE((const void*)d.out != d.x, "ctts_vocoder_conv_h: out must not alias x");
  p.vec = !p.x_f32 && d.sxc == 1 && d.Cin % 8 == 0 && d.sxt % 8 == 0 && d.sxb % 8 == 0 && ((uintptr_t)d.x & 15) == 0;
  // 128-row tiles: measured faster than 256-row tiles at both bench shapes (29.4 against 35.9 ms at B = 16 x 1024, DESIGN.md section 8 -
  // four waves per SIMD beat the halved weight traffic).  The result does not depend on the tile height.
  hipStream_t st = (hipStream_t)stream;
  // CTTS_VOCODER_H_BM=256 selects the 256-row tiles for that A/B measurement; read once
  static const int force_bm = [] { const char* e = getenv("CTTS_VOCODER_H_BM"); return e ? atoi(e) : 0; }();
  if (force_bm == 256) vconv_h_launch<256>(p, BN, d.B, st);
  else vconv_h_launch<128>(p, BN, d.B, st);
  CTTS_CHECK_LAUNCH("ctts_vocoder_conv_h");
  return 0;
}

extern "C" int ctts_vocoder_post_h(const uint16_t* x, int B, int T, int C, int k, const float* w, const float* bias, float slope,
                                   float* out, const int32_t* lens, int len_mul, void* stream) {
  return vpost_launch("ctts_vocoder_post_h", reinterpret_cast<const _Float16*>(x), B, T, C, k, w, bias, slope, out, lens, len_mul, stream);
}
