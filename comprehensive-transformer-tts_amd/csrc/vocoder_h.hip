// HiFi-GAN V1 generator, half-precision (fp16) inference mode: the layers of csrc/vocoder.hip with fp16 weights and activations on
// v_mfma_f32_32x32x16_f16, one MFMA term per product (include/ctts.h, "fp16 mode" - the arithmetic contract lives there).
//
// vconv_h_kernel: the implicit GEMM of vconv_kernel (rows = positions of one utterance, N = output columns, K = taps x Cin; the
//   polyphase ConvTranspose1d with its phase scatter; on-load leaky_relu; out = beta * out + alpha * (acc + bias + R); lens / len_mul
//   with tiles anchored at row 0 of each utterance) reshaped for one operand plane:
//   - a workgroup owns BM = 128 positions x BN columns.  A 256-row instantiation (a staged weight block serves twice the positions:
//     16 MFMAs per wave and tap from 12 ds_read_b128 at BN = 128) exists behind CTTS_VOCODER_H_BM=256 and measured SLOWER (DESIGN.md
//     section 8): 190 VGPRs leave two waves per SIMD where the 128-row tile keeps four.  The tile height does not change a single bit:
//     an output element is one lane's accumulator over a K order (32-channel chunk, tap, channel) that no tile shape enters.
//   - the weight K-block (BN x 32 fp16 = 8 KB at BN = 128) is double-buffered in LDS: the next tap's block is fetched into registers
//     before the current tap's MFMAs, stored into the other buffer after them, and ONE barrier per tap orders both (vconv_kernel: two).
//   - LDS per workgroup: (BM + 64) x 64 B input rows + 2 x BN x 64 B weights = 36 KB at 256 x 128, 28 KB at 128 x 128.
//   Input rows are 64 bytes (32 fp16 of one chunk), the four 16-byte pieces XOR-swizzled by (row >> 2) & 3 - the single-plane image of
//   vconv_kernel's split tiles, read by the same ds_read_b128 pattern.
// vpost_h_kernel: conv_post on fp16 input - leaky_relu on load, 7-tap dot product on the VALU in fp32, + bias, tanh, fp32 out; with lens
//   exact zeros from row Tb on.
#include "ctts_common.h"
#include <stdlib.h>

namespace {

typedef float vh_floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 vh_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int vh_u32x4 __attribute__((ext_vector_type(4)));

constexpr int VH_HALO_MAX = 64;            // (taps - 1) x dil: V1's largest is (11 - 1) x 5 = 50
constexpr float VH_MAX = 65504.f;          // largest finite fp16

struct VhParams {
  const void* x; long sxb, sxt, sxc; int x_f32;
  int T, Cin, cin_pad, taps, dil, in_off, row_off, Mrows, N, Cout, u, pad, Tout;
  int act_in; float slope; int vec;
  const uint16_t* w; const float* bias; const _Float16* R; _Float16* out;
  float alpha, beta;
  const int* lens; int len_mul, mextra;     // ragged: utterance b's input has min(lens[b] len_mul, T) rows; Mrows = T + mextra
};

// rows of utterance b's signal at a layer whose dense length is T: min(max(lens[b], 0) len_mul, T); lens == NULL: T (wave-uniform)
__device__ __forceinline__ int vh_rows(const int* lens, int b, int len_mul, int T) {
  if (!lens) return T;
  const long n = (long)max(lens[b], 0) * len_mul;
  return n < (long)T ? (int)n : T;
}

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
  constexpr int AROWS = BM + VH_HALO_MAX;
  constexpr int B_BYTES = BN * 64;                    // one staged weight K-block
  constexpr int B_CHUNKS = BN * 4;                    // its 16-byte pieces
  constexpr int B_PER_T = (B_CHUNKS + 255) / 256;
  __shared__ __attribute__((aligned(16))) unsigned char smem[AROWS * 64 + 2 * B_BYTES];
  unsigned char* sA = smem;
  unsigned char* sB = smem + AROWS * 64;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, m0 = blockIdx.x * BM, col0 = blockIdx.y * BN;
  const int wm0 = (wave / WAVES_N) * (MT * 32), wn0 = (wave % WAVES_N) * (NT * 32);
  // ragged (include/ctts.h): the utterance's own length replaces T everywhere below; a tile at or beyond its end has nothing to do
  const int Tb = vh_rows(p.lens, b, p.len_mul, p.T), Mb = Tb + p.mextra, Toutb = p.u ? Tb * p.u : Tb;
  if (Tb == 0 || m0 >= Mb) return;
  const int p0 = p.row_off + m0;                      // position of tile row 0
  const int nchunks = p.cin_pad >> 5, taps = p.taps;
  const long kp = (long)taps * p.cin_pad;             // packed weight row length (fp16 elements)
  const int arows = BM + (taps - 1) * p.dil;

  vh_floatx16 acc[MT][NT];
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
      const int ti = p0 + p.in_off + i;
      vh_f16x8 hv;
#pragma unroll
      for (int e = 0; e < 8; ++e) hv[e] = (_Float16)0.f;
      if (ti >= 0 && ti < Tb) {
        const long roff = (long)b * p.sxb + (long)ti * p.sxt;
        if (p.vec) {
          if (cbase < p.Cin) hv = *reinterpret_cast<const vh_f16x8*>(reinterpret_cast<const _Float16*>(p.x) + roff + cbase);   // act_in = 0: taken as it is - no rounding, so no saturation (include/ctts.h)
          if (p.act_in) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float v = (float)hv[e];
              hv[e] = vh_round(v > 0.f ? v : v * p.slope);
            }
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (cbase + e < p.Cin) {
              const long off = roff + (long)(cbase + e) * p.sxc;
              float v = p.x_f32 ? reinterpret_cast<const float*>(p.x)[off] : (float)reinterpret_cast<const _Float16*>(p.x)[off];
              if (p.act_in) v = v > 0.f ? v : v * p.slope;
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
      compute(tap * p.dil, tap & 1);
      if (tap + 1 < taps) {
        store_b((tap + 1) & 1);            // the buffer tap - 1 was read from: every wave left that read before the previous barrier
        __syncthreads();
      }
    }
  }

  // epilogue: element (row wm0 + 32 i + (r & 3) + 8 (r >> 2) + 4 h, column wn0 + 32 j + l31) of the wave's tiles
  const long obase = (long)b * p.Tout * p.Cout;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = col0 + wn0 + j * 32 + l31;
    if (n >= p.N) continue;
    int ph = 0, co = n;
    if (p.u) { ph = n / p.Cout; co = n - ph * p.Cout; }
    const float bv = p.bias ? p.bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ml = wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m0 + ml >= Mb) continue;
        const int pos = p0 + ml;
        const int to = p.u ? pos * p.u + ph - p.pad : pos;
        if (to < 0 || to >= Toutb) continue;
        const long idx = obase + (long)to * p.Cout + co;
        float v = acc[i][j][r] + bv;
        if (p.R) v += (float)p.R[idx];
        v *= p.alpha;
        if (p.beta != 0.f) v = p.beta * (float)p.out[idx] + v;
        p.out[idx] = vh_round(v);
      }
  }
}

constexpr int VPH_ROWS = 256, VPH_PITCH = 33;

// out[b, 0, t] = tanh(bias + sum_{tap, c} leaky_relu(float(x[b, t + tap - (k - 1) / 2, c]), slope) w[tap][c]); x fp16 [B, T, C] dense
// ragged (lens != NULL): rows at or beyond Tb = min(lens[b] len_mul, T) read as zero and out[b, 0, Tb ..] = 0
__global__ __launch_bounds__(256) void vpost_h_kernel(const _Float16* __restrict__ x, int T, int C, int k, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float slope, float* __restrict__ out,
                                                      const int* __restrict__ lens, int len_mul) {
  extern __shared__ float xs[];
  const int b = blockIdx.y, t0 = blockIdx.x * VPH_ROWS, tid = threadIdx.x, half = (k - 1) / 2;
  const int rows = VPH_ROWS + k - 1;
  const _Float16* xb = x + (long)b * T * C;
  const int Tb = vh_rows(lens, b, len_mul, T);
  if (t0 >= Tb) {                          // a tile beyond the utterance's end: the zeros of the result, nothing staged
    if (t0 + tid < T) out[(long)b * T + t0 + tid] = 0.f;
    return;
  }
  float acc = 0.f;
  for (int c0 = 0; c0 < C; c0 += 32) {
    __syncthreads();
    for (int e = tid; e < rows * 32; e += 256) {
      const int r = e >> 5, c = e & 31, t = t0 - half + r;
      float v = 0.f;
      if (t >= 0 && t < Tb && c0 + c < C) {
        v = (float)xb[(long)t * C + c0 + c];
        v = v > 0.f ? v : v * slope;
      }
      xs[r * VPH_PITCH + c] = v;
    }
    __syncthreads();
    const int cn = min(32, C - c0);
    for (int tap = 0; tap < k; ++tap) {
      const float* wr = w + (long)tap * C + c0;
      const float* xr = xs + (tid + tap) * VPH_PITCH;
      for (int c = 0; c < cn; ++c) acc = fmaf(xr[c], wr[c], acc);
    }
  }
  const int t = t0 + tid;
  if (t < T) out[(long)b * T + t] = t < Tb ? tanhf(acc + bias[0]) : 0.f;
}

template <int BM>
void vconv_h_launch(const VhParams& p, int BN, int B, hipStream_t st) {
  dim3 grid((p.Mrows + BM - 1) / BM, (p.N + BN - 1) / BN, B);
  if (BN == 128) hipLaunchKernelGGL((vconv_h_kernel<BM, 128>), grid, dim3(256), 0, st, p);
  else if (BN == 64) hipLaunchKernelGGL((vconv_h_kernel<BM, 64>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((vconv_h_kernel<BM, 32>), grid, dim3(256), 0, st, p);
}

}  // namespace

extern "C" int ctts_vocoder_conv_h(const ctts_vconv_h_desc* dp, void* stream) {
  CTTS_REQUIRE(dp, "ctts_vocoder_conv_h: NULL descriptor");
  const ctts_vconv_h_desc& d = *dp;
  CTTS_REQUIRE(d.x && d.w && d.out, "ctts_vocoder_conv_h: x, w and out are required");
  CTTS_REQUIRE(d.B >= 1 && d.T >= 1 && d.Cin >= 1 && d.Cout >= 1 && d.k >= 1, "ctts_vocoder_conv_h: bad shape B=%d T=%d Cin=%d Cout=%d k=%d",
               d.B, d.T, d.Cin, d.Cout, d.k);
  VhParams p{};
  p.x = d.x; p.sxb = d.sxb; p.sxt = d.sxt; p.sxc = d.sxc; p.x_f32 = d.x_f32 != 0;
  p.T = d.T; p.Cin = d.Cin; p.cin_pad = (d.Cin + 31) / 32 * 32; p.Cout = d.Cout;
  p.act_in = d.act_in; p.slope = d.slope;
  p.w = d.w; p.bias = d.bias; p.R = reinterpret_cast<const _Float16*>(d.R); p.out = reinterpret_cast<_Float16*>(d.out);
  p.alpha = d.alpha; p.beta = d.beta;
  CTTS_REQUIRE(!d.lens || d.len_mul >= 1, "ctts_vocoder_conv_h: lens needs len_mul >= 1 (len_mul=%d)", d.len_mul);
  p.lens = d.lens; p.len_mul = d.len_mul;
  const int u = d.transposed_u;
  if (u == 0) {
    CTTS_REQUIRE(d.k % 2 == 1 && d.dil >= 1, "ctts_vocoder_conv_h: Conv1d needs an odd k and dil >= 1 (k=%d dil=%d)", d.k, d.dil);
    p.taps = d.k; p.dil = d.dil; p.in_off = -(d.k - 1) * d.dil / 2; p.row_off = 0; p.Mrows = d.T;
    p.N = d.Cout; p.u = 0; p.pad = 0; p.Tout = d.T;
  } else {
    CTTS_REQUIRE(u >= 1 && d.k % u == 0 && (d.k - u) % 2 == 0,
                 "ctts_vocoder_conv_h: ConvTranspose1d needs k %% u == 0 and (k - u) even (k=%d u=%d)", d.k, u);
    const int pad = (d.k - u) / 2, J = d.k / u;
    // q rows whose phases reach [0, T u): q u + r - pad >= 0 for some r < u, q u - pad < T u
    const int qlo = pad / u, qhi = d.T + (pad + u - 1) / u;
    p.taps = J; p.dil = 1; p.in_off = -(J - 1); p.row_off = qlo; p.Mrows = qhi - qlo;
    p.N = u * d.Cout; p.u = u; p.pad = pad; p.Tout = d.T * u;
  }
  p.mextra = p.Mrows - d.T;               // the grid is sized by the padded T: no host read of lens
  CTTS_REQUIRE((p.taps - 1) * p.dil <= VH_HALO_MAX, "ctts_vocoder_conv_h: halo (taps - 1) x dil = %d exceeds %d", (p.taps - 1) * p.dil,
               VH_HALO_MAX);
  CTTS_REQUIRE(((uintptr_t)d.w & 15) == 0, "ctts_vocoder_conv_h: packed weights must be 16-byte aligned");
  CTTS_REQUIRE(((uintptr_t)d.out & 1) == 0 && ((uintptr_t)d.R & 1) == 0 && ((uintptr_t)d.x & (p.x_f32 ? 3 : 1)) == 0,
               "ctts_vocoder_conv_h: misaligned x, R or out");
  CTTS_REQUIRE((const void*)d.out != d.x, "ctts_vocoder_conv_h: out must not alias x");
  p.vec = !p.x_f32 && d.sxc == 1 && d.Cin % 8 == 0 && d.sxt % 8 == 0 && d.sxb % 8 == 0 && ((uintptr_t)d.x & 15) == 0;
  const int BN = p.N % 128 == 0 ? 128 : (p.N % 64 == 0 ? 64 : 32);
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
  CTTS_REQUIRE(x && w && bias && out && B >= 1 && T >= 1 && C >= 1 && k >= 1 && k % 2 == 1,
               "ctts_vocoder_post_h: bad arguments (B=%d T=%d C=%d k=%d)", B, T, C, k);
  CTTS_REQUIRE(!lens || len_mul >= 1, "ctts_vocoder_post_h: lens needs len_mul >= 1 (len_mul=%d)", len_mul);
  const size_t lds = (size_t)(VPH_ROWS + k - 1) * VPH_PITCH * sizeof(float);
  CTTS_REQUIRE(lds <= 64 * 1024, "ctts_vocoder_post_h: k=%d too large", k);
  dim3 grid((T + VPH_ROWS - 1) / VPH_ROWS, B);
  hipLaunchKernelGGL(vpost_h_kernel, grid, dim3(256), lds, (hipStream_t)stream, reinterpret_cast<const _Float16*>(x), T, C, k, w, bias,
                     slope, out, lens, len_mul);
  CTTS_CHECK_LAUNCH("ctts_vocoder_post_h");
  return 0;
}
