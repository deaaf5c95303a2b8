// DeepSpeaker speaker embeddings on the device (include/ctts.h "Speaker embeddings on the device"): the voice span
// and filterbank features of deepspeaker/audio_ds.py, and the ResCNN of deepspeaker/conv_models.py as NHWC implicit-GEMM convolutions.
// The definitions are those of ctts_amd.speaker (module docstring) and tests/speaker_restate.py.
//
//   span_kernel        one workgroup per utterance: the two order statistics of |x| around the 95th percentile by a four-pass radix
//                      select on the bit patterns (non-negative floats order as their bits), the threshold in double, then the lowest and
//                      highest sample above it.  Integer LDS atomics only: the result does not depend on the order of arrival.
//   fbank_kernel       one workgroup per (output frame, utterance): pre-emphasis, a 1024-point FFT in LDS (fft_common.h), the 64 triangular filters and the
//                      per-frame normalisation, all in DOUBLE (2560 frames per batch of 16: the fp64 rate is no concern and the features
//                      leave with one fp32 rounding).
//   conv_mfma_kernel   the implicit GEMM  out[m][n] = sum_k A[m][k] W[k][n],  m = (b, oh, ow), k = (kh, kw, cin), n = cout, on the exact
//                      fp32 MFMA (v_mfma_f32_32x32x2_f32).  A 64 x 64 tile per workgroup of four waves, each a 32 x 32 quadrant; a K block is
//                      32 input channels of one filter tap, which NHWC makes 128 contiguous bytes per output pixel - the patch matrix
//                      never exists in memory.  Shapes with few tiles per image (stage 4: 8 tiles, K = 4608) split K over blockIdx.z; the splits write
//                      their partial tiles and conv_reduce_kernel adds them in index order, so there are no float atomics.
//   conv_direct_kernel Cin = 1 (K <= 25): one thread per output element.
//   head_kernel        mean over time, affine layer, L2 normalisation; one workgroup per utterance, sums in double in index order.
// Every sum has a fixed order: results are bit-identical run to run and a row does not depend on the other rows.
#include "ctts_common.h"
#include "fft_common.h"
#include <math.h>

namespace {

constexpr int SP_SPAN_THREADS = 1024;
constexpr int SP_FRAME = 551, SP_STEP = 221, SP_NFFT = 1024, SP_NFILT = 64, SP_BINS = SP_NFFT / 2 + 1;
constexpr int SP_FB_THREADS = 256;
constexpr double SP_PREEMPH = 0.97;
constexpr double SP_EPS = 2.220446049250313e-16;      // np.finfo(float).eps

__host__ __device__ __forceinline__ int sp_frames(int L) { return L <= SP_FRAME ? 1 : 1 + (L - SP_FRAME + SP_STEP - 1) / SP_STEP; }

// ---------------------------------------------------------------- voice span
// np.percentile(a, 95), method "linear", as numpy evaluates it: the virtual index (n - 1) q (one rounding), the interpolation
// a + (b - a) g, or b - (b - a)(1 - g) from g = 0.5 on.  No contraction into fused multiply-adds: numpy rounds every product.
__device__ __noinline__ void sp_virtual_index(int n, int* k, double* g) {
#pragma clang fp contract(off)
  const double v = (double)(n - 1) * 0.95;
  const double fl = floor(v);
  *g = v - fl;
  *k = v >= (double)(n - 1) ? n - 1 : (v < 0.0 ? 0 : (int)fl);
}
__device__ __noinline__ double sp_lerp(double a, double b, double g) {
#pragma clang fp contract(off)
  const double d = b - a;
  if (g >= 0.5) {
    const double t = 1.0 - g;
    const double p = d * t;
    return b - p;
  }
  const double p = d * g;
  return a + p;
}

__global__ __launch_bounds__(SP_SPAN_THREADS) void span_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens,
                                                               int32_t* __restrict__ first, int32_t* __restrict__ last,
                                                               int32_t* __restrict__ n_frames, int32_t* __restrict__ valid, int N) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_rank, s_cnt, s_next;
  __shared__ int s_first, s_last;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(lens[b], 0), N);
  const unsigned* x = reinterpret_cast<const unsigned*>(wav + (long)b * N);
  if (n == 0) {                                                     // uniform over the workgroup
    if (tid == 0) first[b] = 0, last[b] = 0, n_frames[b] = 0, valid[b] = 0;
    return;
  }
  int k;
  double g;
  sp_virtual_index(n, &k, &g);
  if (tid == 0) s_prefix = 0u, s_rank = (unsigned)k;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    const unsigned long long prefix = s_prefix;
    for (int i = tid; i < n; i += SP_SPAN_THREADS) {
      const unsigned key = x[i] & 0x7fffffffu;
      if (((unsigned long long)key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned rank = s_rank, d = 0;
      while (d < 255u && rank >= hist[d]) rank -= hist[d], ++d;      // the counts of the matching keys sum to more than rank
      s_rank = rank;
      s_prefix = (s_prefix << 8) | d;
    }
    __syncthreads();
  }
  const unsigned vk = s_prefix;                                      // bits of a[k]
  if (tid == 0) s_cnt = 0u, s_next = 0xffffffffu, s_first = 0x7fffffff, s_last = -1;
  __syncthreads();
  {
    unsigned c = 0, mn = 0xffffffffu;
    for (int i = tid; i < n; i += SP_SPAN_THREADS) {
      const unsigned key = x[i] & 0x7fffffffu;
      if (key <= vk) ++c;
      else mn = min(mn, key);
    }
    atomicAdd(&s_cnt, c);
    atomicMin(&s_next, mn);
  }
  __syncthreads();
  const unsigned vn = (k + 1 <= n - 1 && (unsigned)(k + 1) >= s_cnt) ? s_next : vk;       // bits of a[min(k + 1, n - 1)]
  const double thr = sp_lerp((double)__uint_as_float(vk), (double)__uint_as_float(vn), g);
  {
    int lo = 0x7fffffff, hi = -1;
    for (int i = tid; i < n; i += SP_SPAN_THREADS) {
      if ((double)__uint_as_float(x[i] & 0x7fffffffu) > thr) lo = min(lo, i), hi = max(hi, i);
    }
    if (hi >= 0) atomicMin(&s_first, lo), atomicMax(&s_last, hi);
  }
  __syncthreads();
  if (tid == 0) {
    const int f = s_last >= 0 ? s_first : 0, l = s_last >= 0 ? s_last : 0;
    const int ok = l - f >= 1 ? 1 : 0;
    first[b] = f;
    last[b] = l;
    valid[b] = ok;
    n_frames[b] = ok ? sp_frames(l - f) : 0;
  }
}

// ---------------------------------------------------------------- filterbank features
__global__ __launch_bounds__(SP_FB_THREADS) void fbank_kernel(const float* __restrict__ wav, const int32_t* __restrict__ first,
                                                              const int32_t* __restrict__ last, const int32_t* __restrict__ valid,
                                                              const int32_t* __restrict__ bins, const int32_t* __restrict__ offsets,
                                                              float* __restrict__ out, int N, int OF, int centre) {
  __shared__ double2 a[SP_NFFT];
  __shared__ double2 tw[SP_NFFT / 2];
  __shared__ double P[SP_BINS + 1];
  __shared__ double fb[SP_NFILT];
  const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  const int s0 = min(max(first[b], 0), N);
  const int L = min(max(last[b] - s0, 0), N - s0);
  const int F = (valid[b] != 0 && L >= 1) ? sp_frames(L) : 0;
  const int rmax = max(F - OF, 0);
  const int r = min(max(offsets ? offsets[b] : (centre ? rmax / 2 : 0), 0), rmax);
  const int f = r + j;
  float* o = out + ((long)b * OF + j) * SP_NFILT;
  if (f >= F) {                                                     // uniform: a padding row
    if (tid < SP_NFILT) o[tid] = 0.f;
    return;
  }
  const float* x = wav + (long)b * N + s0;
  for (int i = tid; i < SP_NFFT; i += SP_FB_THREADS) {
    const long pos = (long)f * SP_STEP + i;
    double v = 0.0;
    if (i < SP_FRAME && pos < L) {
      v = (double)x[pos];
      if (pos > 0) v -= SP_PREEMPH * (double)x[pos - 1];
    }
    a[ctts_dfft_slot<SP_NFFT>(i)] = make_double2(v, 0.0);
  }
  ctts_dfft_fill_twiddles<SP_NFFT, SP_FB_THREADS>(tw, tid);
  __syncthreads();
  for (int s = 0; s < ctts_log2<SP_NFFT>::value; ++s) ctts_dfft_pass<SP_NFFT, SP_FB_THREADS>(a, tw, s, tid);
  for (int i = tid; i < SP_BINS; i += SP_FB_THREADS) P[i] = (a[i].x * a[i].x + a[i].y * a[i].y) / (double)SP_NFFT;
  __syncthreads();
  if (tid < SP_NFILT) {
    const int b0 = min(max(bins[tid], 0), SP_BINS), b1 = min(max(bins[tid + 1], b0), SP_BINS), b2 = min(max(bins[tid + 2], b1), SP_BINS);
    double s = 0.0;
    for (int i = b0; i < b1; ++i) s += P[i] * ((double)(i - b0) / (double)(b1 - b0));
    for (int i = b1; i < b2; ++i) s += P[i] * ((double)(b2 - i) / (double)(b2 - b1));
    fb[tid] = s == 0.0 ? SP_EPS : s;
  }
  __syncthreads();
  if (tid < SP_NFILT) {
    double m = 0.0;
    for (int i = 0; i < SP_NFILT; ++i) m += fb[i];
    m /= (double)SP_NFILT;
    double q = 0.0;
    for (int i = 0; i < SP_NFILT; ++i) q += (fb[i] - m) * (fb[i] - m);
    const double sd = sqrt(q / (double)SP_NFILT);
    o[tid] = (float)((fb[tid] - m) / fmax(sd, 1e-12));
  }
}

// ---------------------------------------------------------------- NHWC convolution
struct ConvGeom {
  int B, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo;
  long M;
};

// TF 'same': out = ceil(n / s), total = max((out - 1) s + k - n, 0), before = total / 2 (the odd cell goes after)
static bool conv_geometry(int B, int H, int W, int Cin, int Cout, int geom, ConvGeom* g) {
  if (B < 1 || H < 1 || W < 1 || Cout < 64 || Cout % 64 || !(Cin == 1 || (Cin >= 64 && Cin % 64 == 0)) || (geom != 0 && geom != 1)) return false;
  const int k = geom == 0 ? 5 : 3, s = geom == 0 ? 2 : 1;
  g->B = B, g->H = H, g->W = W, g->Cin = Cin, g->Cout = Cout, g->KH = k, g->KW = k, g->stride = s;
  g->Ho = (H + s - 1) / s, g->Wo = (W + s - 1) / s;
  const int th = (g->Ho - 1) * s + k - H, tw = (g->Wo - 1) * s + k - W;
  g->pad_t = (th > 0 ? th : 0) / 2, g->pad_l = (tw > 0 ? tw : 0) / 2;
  g->M = (long)B * g->Ho * g->Wo;
  const long lim = 1L << 31;
  return g->M * Cout < lim && (long)B * H * W * Cin < lim && g->M < (1L << 30);
}

constexpr int CV_BM = 64, CV_BN = 64, CV_BK = 32, CV_THREADS = 256;
constexpr int CV_SA = CV_BK + 4;        // A rows of 36 words: 16-byte aligned stores, the 32 rows x 2 k of a fragment read 2-way at worst
constexpr int CV_SB = CV_BN + 32;       // W rows of 96 words: the 2 k x 32 columns of a fragment read fall on 64 different banks
constexpr int CV_MAX_SPLIT = 32, CV_MIN_KB = 18, CV_FILL = 64;

// K blocks of a launch, and how many of them one split takes.  The plan is a function of ONE image's shape, never of B: the order in which
// an output element's products are added - hence its bits - does not depend on the batch around it.  An image with fewer than CV_FILL
// tiles splits K until it has that many workgroups, a split keeping at least CV_MIN_KB K blocks (K = 576): at B = 16 stage 2 runs
// 320 tiles x 2 splits, stage 3 160 x 4, stage 4 80 x 8 - two to three workgroups per CU, which is what hides the global loads of a
// kernel that holds one LDS stage.  Measured on the canonical batch against (CV_FILL 32, CV_MIN_KB 4): stage 4 0.646 -> 0.440 ms.
static void conv_split(const ConvGeom& g, int* splits, int* per) {
  const int nkb = g.KH * g.KW * (g.Cin / CV_BK);
  const int tiles = ((g.Ho * g.Wo + CV_BM - 1) / CV_BM) * (g.Cout / CV_BN);
  int s = 1;
  if (tiles < CV_FILL) {
    s = (CV_FILL + tiles - 1) / tiles;
    if (s > CV_MAX_SPLIT) s = CV_MAX_SPLIT;
    if (s > nkb / CV_MIN_KB) s = nkb / CV_MIN_KB;
    if (s < 1) s = 1;
  }
  *per = (nkb + s - 1) / s;
  *splits = (nkb + *per - 1) / *per;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float cv_clip(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

__global__ __launch_bounds__(CV_THREADS) void conv_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ res,
                                                               float* __restrict__ out, float* __restrict__ part, ConvGeom g, int per,
                                                               int splits, int mode, float lo, float hi) {
  __shared__ __attribute__((aligned(16))) float As[CV_BM * CV_SA];
  __shared__ __attribute__((aligned(16))) float Bs[CV_BK * CV_SB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long m0 = (long)blockIdx.x * CV_BM;
  const int n0 = blockIdx.y * CV_BN;
  const int cpb = g.Cin / CV_BK;                                     // K blocks per tap
  const int nkb = g.KH * g.KW * cpb;
  const int kb0 = blockIdx.z * per, kb1 = min(kb0 + per, nkb);

  // this thread's two A rows (ar, ar + 32) and channel quad, its two W rows (br, br + 16) and column quad
  const int ar = tid >> 3, ac = (tid & 7) * 4;
  const int br = tid >> 4, bc = (tid & 15) * 4;
  int ih0[2], iw0[2];
  long xb[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const long m = m0 + ar + 32 * u;
    if (m < g.M) {
      const int ow = (int)(m % g.Wo), oh = (int)((m / g.Wo) % g.Ho), bb = (int)(m / ((long)g.Wo * g.Ho));
      ih0[u] = oh * g.stride - g.pad_t, iw0[u] = ow * g.stride - g.pad_l;
      xb[u] = (long)bb * g.H * g.W;
    } else {
      ih0[u] = -(1 << 20), iw0[u] = 0, xb[u] = 0;                   // every tap falls outside: the row stays zero
    }
  }
  float4 pa[2], pb[2];
  auto fetch = [&](int kb) {
    const int tap = kb / cpb, c0 = (kb - tap * cpb) * CV_BK;
    const int kh = tap / g.KW, kw = tap - kh * g.KW;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int ih = ih0[u] + kh, iw = iw0[u] + kw;
      pa[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
        pa[u] = *reinterpret_cast<const float4*>(x + (xb[u] + (long)ih * g.W + iw) * g.Cin + c0 + ac);
      pb[u] = *reinterpret_cast<const float4*>(w + ((long)tap * g.Cin + c0 + br + 16 * u) * g.Cout + n0 + bc);
    }
  };
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const float* af = As + (wm + (lane & 31)) * CV_SA + (lane >> 5);
  const float* bf = Bs + (lane >> 5) * CV_SB + wn + (lane & 31);
  if (kb0 < kb1) fetch(kb0);
  for (int kb = kb0; kb < kb1; ++kb) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      *reinterpret_cast<float4*>(As + (ar + 32 * u) * CV_SA + ac) = pa[u];
      *reinterpret_cast<float4*>(Bs + (br + 16 * u) * CV_SB + bc) = pb[u];
    }
    __syncthreads();
    if (kb + 1 < kb1) fetch(kb + 1);                                // in flight under the MFMAs below
#pragma unroll
    for (int kk = 0; kk < CV_BK / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[2 * kk], bf[2 * kk * CV_SB], acc, 0, 0, 0);
    __syncthreads();
  }
  const int n = n0 + wn + (lane & 31);
  const float bn = bias[n];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long m = m0 + wm + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
    if (m >= g.M) continue;
    if (splits > 1) {
      part[((long)blockIdx.z * g.M + m) * g.Cout + n] = acc[i];
    } else {
      float v = cv_clip(acc[i] + bn, lo, hi);
      if (mode) v = cv_clip(v + res[m * g.Cout + n], lo, hi);
      out[m * g.Cout + n] = v;
    }
  }
}

__global__ __launch_bounds__(256) void conv_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                          const float* __restrict__ res, float* __restrict__ out, long total, int Cout,
                                                          int splits, int mode, float lo, float hi) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= total) return;                                           // total = M Cout is a multiple of 64
  float4 s = *reinterpret_cast<const float4*>(part + i);
  for (int k = 1; k < splits; ++k) {                                // index order
    const float4 p = *reinterpret_cast<const float4*>(part + (long)k * total + i);
    s.x += p.x, s.y += p.y, s.z += p.z, s.w += p.w;
  }
  const float4 bq = *reinterpret_cast<const float4*>(bias + (int)(i % Cout));
  float4 v = make_float4(cv_clip(s.x + bq.x, lo, hi), cv_clip(s.y + bq.y, lo, hi), cv_clip(s.z + bq.z, lo, hi), cv_clip(s.w + bq.w, lo, hi));
  if (mode) {
    const float4 r = *reinterpret_cast<const float4*>(res + i);
    v = make_float4(cv_clip(v.x + r.x, lo, hi), cv_clip(v.y + r.y, lo, hi), cv_clip(v.z + r.z, lo, hi), cv_clip(v.w + r.w, lo, hi));
  }
  *reinterpret_cast<float4*>(out + i) = v;
}

__global__ __launch_bounds__(256) void conv_direct_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, const float* __restrict__ res,
                                                          float* __restrict__ out, ConvGeom g, int mode, float lo, float hi) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.M * g.Cout) return;
  const int n = (int)(i % g.Cout);
  const long m = i / g.Cout;
  const int ow = (int)(m % g.Wo), oh = (int)((m / g.Wo) % g.Ho), bb = (int)(m / ((long)g.Wo * g.Ho));
  const float* xp = x + (long)bb * g.H * g.W;
  float acc = 0.f;
  for (int kh = 0; kh < g.KH; ++kh) {
    const int ih = oh * g.stride - g.pad_t + kh;
    if (ih < 0 || ih >= g.H) continue;
    for (int kw = 0; kw < g.KW; ++kw) {
      const int iw = ow * g.stride - g.pad_l + kw;
      if (iw < 0 || iw >= g.W) continue;
      acc = fmaf(xp[(long)ih * g.W + iw], w[(kh * g.KW + kw) * g.Cout + n], acc);
    }
  }
  float v = cv_clip(acc + bias[n], lo, hi);
  if (mode) v = cv_clip(v + res[i], lo, hi);
  out[i] = v;
}

// ---------------------------------------------------------------- head: time mean, affine, L2 normalisation
constexpr int HD_THREADS = 512;

__global__ __launch_bounds__(HD_THREADS) void head_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, const int32_t* __restrict__ valid,
                                                          float* __restrict__ out, int T, int F, int E) {
  extern __shared__ double hd_lds[];                                // mean [F], y [E], red [HD_THREADS]
  double* mean = hd_lds;
  double* y = hd_lds + F;
  double* red = y + E;
  const int b = blockIdx.x, tid = threadIdx.x;
  float* o = out + (long)b * E;
  if (valid && valid[b] == 0) {                                     // uniform
    for (int e = tid; e < E; e += HD_THREADS) o[e] = 0.f;
    return;
  }
  const float* xb = x + (long)b * T * F;
  for (int f = tid; f < F; f += HD_THREADS) {
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += (double)xb[(long)t * F + f];
    mean[f] = s / (double)T;
  }
  __syncthreads();
  double sq = 0.0;
  for (int e = tid; e < E; e += HD_THREADS) {
    double s = (double)bias[e];
    for (int f = 0; f < F; ++f) s = fma(mean[f], (double)w[(long)f * E + e], s);
    y[e] = s;
    sq += s * s;
  }
  red[tid] = sq;
  __syncthreads();
  for (int h = HD_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  const double nrm = fmax(sqrt(red[0]), 1e-12);
  for (int e = tid; e < E; e += HD_THREADS) o[e] = (float)(y[e] / nrm);
}

}  // namespace

extern "C" {

int ctts_speaker_frames(int span) { return span < 1 ? 0 : sp_frames(span); }

int ctts_speaker_span(const float* wav, const int32_t* lens, int32_t* first, int32_t* last, int32_t* n_frames, int32_t* valid, int B, int N,
                      void* stream) {
  CTTS_REQUIRE(wav && lens && first && last && n_frames && valid, "ctts_speaker_span: null pointer");
  CTTS_REQUIRE(B >= 1 && N >= 1 && N <= (1 << 30), "ctts_speaker_span: need B >= 1 and 1 <= N <= 2^30, got %d x %d", B, N);
  hipLaunchKernelGGL(span_kernel, dim3(B), dim3(SP_SPAN_THREADS), 0, (hipStream_t)stream, wav, lens, first, last, n_frames, valid, N);
  CTTS_CHECK_LAUNCH("ctts_speaker_span");
  return 0;
}

int ctts_speaker_fbank(const float* wav, const int32_t* first, const int32_t* last, const int32_t* valid, const int32_t* bins,
                       const int32_t* offsets, float* out, int B, int N, int out_frames, int centre, void* stream) {
  CTTS_REQUIRE(wav && first && last && valid && bins && out, "ctts_speaker_fbank: null pointer");
  CTTS_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && N <= (1 << 30) && out_frames >= 1,
               "ctts_speaker_fbank: need 1 <= B <= 65535, 1 <= N <= 2^30 and out_frames >= 1, got %d x %d, %d frames", B, N, out_frames);
  hipLaunchKernelGGL(fbank_kernel, dim3(out_frames, B), dim3(SP_FB_THREADS), 0, (hipStream_t)stream, wav, first, last, valid, bins, offsets,
                     out, N, out_frames, centre);
  CTTS_CHECK_LAUNCH("ctts_speaker_fbank");
  return 0;
}

size_t ctts_conv2d_nhwc_workspace_bytes(int B, int H, int W, int Cin, int Cout, int geom) {
  ConvGeom g;
  if (!conv_geometry(B, H, W, Cin, Cout, geom, &g) || Cin == 1) return 0;
  int splits, per;
  conv_split(g, &splits, &per);
  return splits > 1 ? sizeof(float) * (size_t)splits * (size_t)g.M * (size_t)Cout : 0;
}

int ctts_conv2d_nhwc(const float* x, const float* w, const float* bias, const float* res, float* out, int B, int H, int W, int Cin, int Cout,
                     int geom, int mode, float lo, float hi, void* workspace, void* stream) {
  ConvGeom g;
  CTTS_REQUIRE(x && w && bias && out, "ctts_conv2d_nhwc: null pointer");
  CTTS_REQUIRE(mode == 0 || (mode == 1 && res), "ctts_conv2d_nhwc: mode must be 0, or 1 with a residual, got %d", mode);
  CTTS_REQUIRE(conv_geometry(B, H, W, Cin, Cout, geom, &g),
               "ctts_conv2d_nhwc: need B, H, W >= 1, Cin 1 or a multiple of 64, Cout a multiple of 64, geometry 0 (5x5 stride 2) or 1 (3x3 "
               "stride 1) and fewer than 2^31 input and output elements, got B %d H %d W %d Cin %d Cout %d geometry %d", B, H, W, Cin, Cout, geom);
  CTTS_REQUIRE(!(((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)out | (uintptr_t)res | (uintptr_t)workspace) & 15),
               "ctts_conv2d_nhwc: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (Cin == 1) {
    const long total = g.M * Cout;
    hipLaunchKernelGGL(conv_direct_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, w, bias, res, out, g, mode, lo, hi);
    CTTS_CHECK_LAUNCH("ctts_conv2d_nhwc");
    return 0;
  }
  int splits, per;
  conv_split(g, &splits, &per);
  CTTS_REQUIRE(splits == 1 || workspace, "ctts_conv2d_nhwc: this shape splits K %d ways and needs its workspace", splits);
  const dim3 grid((unsigned)((g.M + CV_BM - 1) / CV_BM), Cout / CV_BN, splits);
  CTTS_REQUIRE(grid.y <= 65535, "ctts_conv2d_nhwc: Cout %d is too wide", Cout);
  hipLaunchKernelGGL(conv_mfma_kernel, grid, dim3(CV_THREADS), 0, st, x, w, bias, res, out, (float*)workspace, g, per, splits, mode, lo, hi);
  CTTS_CHECK_LAUNCH("ctts_conv2d_nhwc");
  if (splits > 1) {
    const long total = g.M * Cout;
    hipLaunchKernelGGL(conv_reduce_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, st, (const float*)workspace, bias, res, out,
                       total, Cout, splits, mode, lo, hi);
    CTTS_CHECK_LAUNCH("ctts_conv2d_nhwc");
  }
  return 0;
}

int ctts_speaker_head(const float* x, const float* w, const float* bias, const int32_t* valid, float* out, int B, int T, int F, int E,
                      void* stream) {
  CTTS_REQUIRE(x && w && bias && out, "ctts_speaker_head: null pointer");
  CTTS_REQUIRE(B >= 1 && T >= 1 && F >= 1 && E >= 1 && F + E <= 7168, "ctts_speaker_head: need B, T, F, E >= 1 and F + E <= 7168, got %d %d %d %d",
               B, T, F, E);
  const size_t lds = sizeof(double) * (size_t)(F + E + HD_THREADS);
  hipLaunchKernelGGL(head_kernel, dim3(B), dim3(HD_THREADS), lds, (hipStream_t)stream, x, w, bias, valid, out, T, F, E);
  CTTS_CHECK_LAUNCH("ctts_speaker_head");
  return 0;
}

}  // extern "C"
