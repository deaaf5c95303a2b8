// What the fp32 (vocoder.hip) and fp16 (vocoder_h.hip) HiFi-GAN kernels share: the layer geometry, the epilogue walk and conv_post.
// The conv main loops (staging, LDS layout, MFMA order) differ by measurement and stay in their files.
// Everything here has internal linkage: the library's exports are those of include/ctts.h.
#pragma once
#include "ctts_common.h"
#include "fft_common.h"                    // ctts_reflect_index

namespace {

typedef float vc_floatx16 __attribute__((ext_vector_type(16)));

constexpr int VC_HALO_MAX = 64;            // (taps - 1) x dil: V1's largest is (11 - 1) x 5 = 50

// One layer as both kernels see it.  Conv1d(k, dil): taps = k rows dil apart from in_off = -(k - 1) dil / 2, N = Cout columns.
// ConvTranspose1d(stride u, kernel K, pad (K - u) / 2) is the polyphase form: output t = q u + r - pad = sum_j x[q - j] W[:, :, r + j u]
// (j < K / u), a K/u-tap stride-1 conv over INPUT time whose N = u x Cout columns hold all phases (column r Cout + co); the epilogue
// scatters row q's phases to output rows q u + r - pad and drops those outside [0, T u).
struct VcGeom {
  int T, Cin, cin_pad, taps, dil, in_off, row_off, Mrows, N, Cout, u, pad, Tout, mextra;
  const int* lens; int len_mul;             // ragged: utterance b's input has min(lens[b] len_mul, T) rows; Mrows = T + mextra
  int act_in; float slope, alpha, beta;
  const float* bias;
};

// The shape checks and geometry of ctts_vocoder_conv / ctts_vocoder_conv_h (`what`: the entry point's name, for the messages).
// Fills every field of g but act_in / slope / alpha / beta / bias and picks the column tile BN.
inline int vc_geometry(const char* what, int B, int T, int Cin, int Cout, int k, int dil, int transposed_u, const int* lens, int len_mul,
                       VcGeom& g, int& BN) {
  CTTS_REQUIRE(B >= 1 && T >= 1 && Cin >= 1 && Cout >= 1 && k >= 1, "%s: bad shape B=%d T=%d Cin=%d Cout=%d k=%d", what, B, T, Cin, Cout, k);
  g.T = T; g.Cin = Cin; g.cin_pad = (Cin + 31) / 32 * 32; g.Cout = Cout;
  CTTS_REQUIRE(!lens || len_mul >= 1, "%s: lens needs len_mul >= 1 (len_mul=%d)", what, len_mul);
  g.lens = lens; g.len_mul = len_mul;
  const int u = transposed_u;
  if (u == 0) {
    CTTS_REQUIRE(k % 2 == 1 && dil >= 1, "%s: Conv1d needs an odd k and dil >= 1 (k=%d dil=%d)", what, k, dil);
    g.taps = k; g.dil = dil; g.in_off = -(k - 1) * dil / 2; g.row_off = 0; g.Mrows = T;
    g.N = Cout; g.u = 0; g.pad = 0; g.Tout = T;
  } else {
    CTTS_REQUIRE(u >= 1 && k % u == 0 && (k - u) % 2 == 0, "%s: ConvTranspose1d needs k %% u == 0 and (k - u) even (k=%d u=%d)", what, k, u);
    const int pad = (k - u) / 2, J = k / u;
    // q rows whose phases reach [0, T u): q u + r - pad >= 0 for some r < u, q u - pad < T u
    const int qlo = pad / u, qhi = T + (pad + u - 1) / u;
    g.taps = J; g.dil = 1; g.in_off = -(J - 1); g.row_off = qlo; g.Mrows = qhi - qlo;
    g.N = u * Cout; g.u = u; g.pad = pad; g.Tout = T * u;
  }
  g.mextra = g.Mrows - T;                  // the grid is sized by the padded T: no host read of lens
  CTTS_REQUIRE((g.taps - 1) * g.dil <= VC_HALO_MAX, "%s: halo (taps - 1) x dil = %d exceeds %d", what, (g.taps - 1) * g.dil, VC_HALO_MAX);
  BN = g.N % 128 == 0 ? 128 : (g.N % 64 == 0 ? 64 : 32);
  return 0;
}

inline dim3 vc_grid(const VcGeom& g, int BM, int BN, int B) { return dim3((g.Mrows + BM - 1) / BM, (g.N + BN - 1) / BN, B); }

// rows of utterance b's signal at a layer whose dense length is T: min(max(lens[b], 0) len_mul, T); lens == NULL: T (wave-uniform)
__device__ __forceinline__ int vc_rows(const int* lens, int b, int len_mul, int T) {
  if (!lens) return T;
  const long n = (long)max(lens[b], 0) * len_mul;
  return n < (long)T ? (int)n : T;
}

// Epilogue walk over a wave's MT x NT accumulator tiles of the workgroup tile at (row m0, column col0) of utterance b: element
// (row wm0 + 32 i + (r & 3) + 8 (r >> 2) + 4 h, column wn0 + 32 j + l31).  Drops columns beyond N and rows beyond the utterance's Mb
// (the phase scatter: output rows outside [0, Toutb)) and hands elem(idx, acc + bias) every element that is stored, idx its offset in
// out (and R) [B, Tout, Cout].  g and the functor's captures are taken BY VALUE: through references the compiler re-derived the
// bounds and the beta test per element (about 3 instructions more for each of a lane's 16 to 64 elements, 1 % of a forward).
template <int MT, int NT, class F>
__device__ __forceinline__ void vc_epilogue(const VcGeom g, const vc_floatx16 (&acc)[MT][NT], int b, int m0, int col0, int wm0, int wn0,
                                            int l31, int h, int Mb, int Toutb, F elem) {
  const int p0 = g.row_off + m0;
  const long obase = (long)b * g.Tout * g.Cout;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = col0 + wn0 + j * 32 + l31;
    if (n >= g.N) continue;
    int ph = 0, co = n;
    if (g.u) { ph = n / g.Cout; co = n - ph * g.Cout; }
    const float bv = g.bias ? g.bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ml = wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m0 + ml >= Mb) continue;
        const int pos = p0 + ml;
        const int to = g.u ? pos * g.u + ph - g.pad : pos;
        if (to < 0 || to >= Toutb) continue;
        elem(obase + (long)to * g.Cout + co, acc[i][j][r] + bv);
      }
  }
}

constexpr int VP_ROWS = 256, VP_PITCH = 33;

// conv_post (Cout = 1, models.py:161-163): leaky_relu on load, k-tap dot product on the VALU in fp32, + bias, tanh, fp32 out.
// out[b, 0, t] = tanh(bias + sum_{tap, c} leaky_relu(float(x[b, t + tap - (k - 1) / 2, c]), slope) w[tap][c]); x [B, T, C] dense
// ragged (lens != NULL): rows at or beyond Tb = min(lens[b] len_mul, T) read as zero and out[b, 0, Tb ..] = 0
// REFLECT (MelGAN's ReflectionPad1d in front of the last conv): a row outside [0, Tb) is read at its reflection about the utterance's ends
template <class TIn, bool REFLECT = false>
__global__ __launch_bounds__(256) void vpost_kernel(const TIn* __restrict__ x, int T, int C, int k, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float slope, float* __restrict__ out,
                                                    const int* __restrict__ lens, int len_mul) {
  extern __shared__ float xs[];
  const int b = blockIdx.y, t0 = blockIdx.x * VP_ROWS, tid = threadIdx.x, half = (k - 1) / 2;
  const int rows = VP_ROWS + k - 1;
  const TIn* xb = x + (long)b * T * C;
  const int Tb = vc_rows(lens, b, len_mul, T);
  if (t0 >= Tb) {                          // a tile beyond the utterance's end: the zeros of the result, nothing staged
    if (t0 + tid < T) out[(long)b * T + t0 + tid] = 0.f;
    return;
  }
  float acc = 0.f;
  for (int c0 = 0; c0 < C; c0 += 32) {
    __syncthreads();
    for (int e = tid; e < rows * 32; e += 256) {
      const int r = e >> 5, c = e & 31;
      int t = t0 - half + r;
      if constexpr (REFLECT) t = ctts_reflect_index(t, Tb);
      float v = 0.f;
      if (t >= 0 && t < Tb && c0 + c < C) {
        v = (float)xb[(long)t * C + c0 + c];
        v = v > 0.f ? v : v * slope;
      }
      xs[r * VP_PITCH + c] = v;
    }
    __syncthreads();
    const int cn = min(32, C - c0);
    for (int tap = 0; tap < k; ++tap) {
      const float* wr = w + (long)tap * C + c0;
      const float* xr = xs + (tid + tap) * VP_PITCH;
      for (int c = 0; c < cn; ++c) acc = fmaf(xr[c], wr[c], acc);
    }
  }
  const int t = t0 + tid;
  if (t < T) out[(long)b * T + t] = t < Tb ? tanhf(acc + bias[0]) : 0.f;
}

// the one launcher behind ctts_vocoder_post / _post_ragged / _post_h (lens == NULL: dense)
template <class TIn, bool REFLECT = false>
int vpost_launch(const char* what, const TIn* x, int B, int T, int C, int k, const float* w, const float* bias, float slope, float* out,
                 const int32_t* lens, int len_mul, void* stream) {
  CTTS_REQUIRE(x && w && bias && out && B >= 1 && T >= 1 && C >= 1 && k >= 1 && k % 2 == 1, "%s: bad arguments (B=%d T=%d C=%d k=%d)", what,
               B, T, C, k);
  CTTS_REQUIRE(!lens || len_mul >= 1, "%s: lens needs len_mul >= 1 (len_mul=%d)", what, len_mul);
  const size_t lds = (size_t)(VP_ROWS + k - 1) * VP_PITCH * sizeof(float);
  CTTS_REQUIRE(lds <= 64 * 1024, "%s: k=%d too large", what, k);
  CTTS_REQUIRE(!REFLECT || T > (k - 1) / 2, "%s: reflection needs T > (k - 1) / 2 (T=%d k=%d)", what, T, k);
  dim3 grid((T + VP_ROWS - 1) / VP_ROWS, B);
  hipLaunchKernelGGL((vpost_kernel<TIn, REFLECT>), grid, dim3(256), lds, (hipStream_t)stream, x, T, C, k, w, bias, slope, out, lens, len_mul);
  CTTS_CHECK_LAUNCH(what);
  return 0;
}

}  // namespace
