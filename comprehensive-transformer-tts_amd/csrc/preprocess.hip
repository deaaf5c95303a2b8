// Dataset preparation on the device (include/ctts.h "Dataset preparation on the device"): the three steps of
// the reference's preprocessor/preprocessor.py that still ran on the host, one utterance at a time.
//
// frame_power_kernel + trim_bounds_kernel - librosa 0.7.2 effects.trim with ref = np.max, restated: one wave per frame sums the squares of the
//   frame's reflect-padded samples in double (16 values per lane at frame_length 1024, a shuffle tree across the wave), then one workgroup
//   per utterance takes the maximum over the frames and the first / last frame above the threshold.
// attn_prior_kernel - the beta-binomial alignment prior (preprocessor.py:551-560 as it is CALLED at :409-413): one workgroup per (phoneme
//   row, utterance), the closed form through lgamma in double, rounded once to float.  Every element of the padded output is written.
// outlier_stats_kernel - remove_outlier (:620-628) and the moments StandardScaler.partial_fit needs: one workgroup per utterance, bitonic
//   sort of its values in LDS, numpy's linear percentiles, the keep mask, then count / sum / M2 in double and min / max over the kept values.
// No float atomics, no inter-workgroup waits, every reduction in a fixed order: results are bit-reproducible and batch-independent.
#include "ctts_common.h"
#include "fft_common.h"
#include <math.h>

namespace {

constexpr int TRIM_FRAMES_PER_WG = 4;                  // one wave per frame
constexpr int OUT_MAX = 4096;                          // values per utterance the outlier kernel sorts in LDS

// ------------------------------------------------------------------------------------------------------------------ silence trim
// mse[b][f] = mean of squares of frame f of utterance b: padded samples [f hop, f hop + frame_length), padded sample p = x[reflect(p -
// frame_length / 2)].  Frames at or beyond 1 + len / hop hold 0 (never consulted).  Only x[0 .. len) is read.
__global__ __launch_bounds__(256) void frame_power_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, float* __restrict__ mse,
                                                           int N, int F, int frame_length, int hop) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * TRIM_FRAMES_PER_WG + wave;                 // wave-uniform
  if (f >= F) return;
  const int len = min(max(lens[b], 0), N);
  float out = 0.f;
  if (len > 0 && f < 1 + len / hop) {
    const float* x = wav + (long)b * N;
    const long base = (long)f * hop - frame_length / 2;
    double acc = 0.0;
    for (int k = lane; k < frame_length; k += 64) {
      const long i = ctts_reflect_index(base + k, (long)len);     // its clamp acts only when len <= frame_length / 2 (outside the domain)
      const double v = (double)x[i];
      acc += v * v;
    }
    out = (float)(ctts_wave_sum_d(acc) / (double)frame_length);
  }
  if (lane == 0) mse[(long)b * F + f] = out;
}

__global__ __launch_bounds__(256) void trim_bounds_kernel(const float* __restrict__ mse, const int32_t* __restrict__ lens, int32_t* __restrict__ start,
                                                           int32_t* __restrict__ end, int N, int F, int hop, float top_db) {
  __shared__ float redf[4];
  __shared__ int redi[8];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const int nf = len > 0 ? 1 + len / hop : 0;
  const float* m = mse + (long)b * F;
  float ref = 0.f;
  for (int f = tid; f < nf; f += 256) ref = fmaxf(ref, m[f]);
  ref = ctts_wave_max(ref);
  if ((tid & 63) == 0) redf[tid >> 6] = ref;
  __syncthreads();
  ref = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
  const double ref_db = 10.0 * log10(fmax(1e-10, (double)ref));
  int first = 0x7fffffff, last = -1;
  for (int f = tid; f < nf; f += 256) {
    const double db = 10.0 * log10(fmax(1e-10, (double)m[f])) - ref_db;
    if (db > -(double)top_db) { first = min(first, f); last = max(last, f); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { first = min(first, __shfl_xor(first, o, 64)); last = max(last, __shfl_xor(last, o, 64)); }
  if ((tid & 63) == 0) { redi[tid >> 6] = first; redi[4 + (tid >> 6)] = last; }
  __syncthreads();
  if (tid == 0) {
    first = min(min(redi[0], redi[1]), min(redi[2], redi[3]));
    last = max(max(redi[4], redi[5]), max(redi[6], redi[7]));
    if (last < 0) { start[b] = 0; end[b] = 0; }
    else { start[b] = (int32_t)min((long)hop * first, (long)len); end[b] = (int32_t)min((long)len, (long)hop * (last + 1)); }
  }
}

// ------------------------------------------------------------------------------------------------------------------ alignment prior
// out[b][s][t] = BetaBinom.pmf(t; n = mel_len, a = sf (s + 1), bb = sf (src_len - s)) for s < src_len, t < mel_len, else 0:
//   log pmf = lgamma(n+1) - lgamma(t+1) - lgamma(n-t+1) + lgamma(t+a) + lgamma(n-t+bb) - lgamma(n+a+bb) - lgamma(a) - lgamma(bb) + lgamma(a+bb)
__global__ __launch_bounds__(256) void attn_prior_kernel(const int32_t* __restrict__ src_lens, const int32_t* __restrict__ mel_lens, float* __restrict__ out,
                                                          int Ts, int Tm, long stride_b, long stride_s, double sf) {
  const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  const int P = min(max(src_lens[b], 0), Ts), n = min(max(mel_lens[b], 0), Tm);
  float* row = out + (long)b * stride_b + (long)s * stride_s;
  if (s >= P) {
    for (int t = tid; t < Tm; t += 256) row[t] = 0.f;
    return;
  }
  const double a = sf * (double)(s + 1), bb = sf * (double)(P - s), dn = (double)n;
  const double c0 = lgamma(dn + 1.0) - lgamma(dn + a + bb) - lgamma(a) - lgamma(bb) + lgamma(a + bb);
  for (int t = tid; t < Tm; t += 256) {
    float v = 0.f;
    if (t < n) {
      const double k = (double)t;
      v = (float)exp(c0 - lgamma(k + 1.0) - lgamma(dn - k + 1.0) + lgamma(k + a) + lgamma(dn - k + bb));
    }
    row[t] = v;
  }
}

// ------------------------------------------------------------------------------------------------------------------ outlier filter + moments
// numpy's default percentile of the sorted values srt[0 .. n): position q (n - 1), linear between the neighbours
__device__ __forceinline__ double percentile_sorted(const float* srt, int n, double q) {
  const double pos = q * (double)(n - 1);
  const int lo = (int)floor(pos), hi = min(lo + 1, n - 1);
  const double fr = pos - (double)lo, x0 = (double)srt[lo], x1 = (double)srt[hi];
  return x0 + (x1 - x0) * fr;
}

__global__ __launch_bounds__(256) void outlier_stats_kernel(const float* __restrict__ values, const int32_t* __restrict__ lens, uint8_t* __restrict__ keep,
                                                             int32_t* __restrict__ count, double* __restrict__ sum, double* __restrict__ m2,
                                                             float* __restrict__ vmin, float* __restrict__ vmax, int L) {
  __shared__ float srt[OUT_MAX];
  __shared__ double red[4];
  __shared__ float redf[8];
  __shared__ int redi[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(lens[b], 0), L);                 // L <= OUT_MAX is checked on the host
  const float* v = values + (long)b * L;
  uint8_t* kp = keep + (long)b * L;
  int M = 1;
  while (M < n) M <<= 1;                                 // <= 4096: at most 12 steps
  for (int i = tid; i < M; i += 256) srt[i] = i < n ? v[i] : INFINITY;
  __syncthreads();
  for (int k = 2; k <= M; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < M; i += 256) {
        const int p = i ^ j;
        if (p > i) {
          const float x = srt[i], y = srt[p];
          const bool up = (i & k) == 0;
          if (up ? (x > y) : (x < y)) { srt[i] = y; srt[p] = x; }
        }
      }
      __syncthreads();
    }
  }
  double lower = 0.0, upper = 0.0;
  if (n > 0) {
    const double p25 = percentile_sorted(srt, n, 0.25), p75 = percentile_sorted(srt, n, 0.75);
    lower = p25 - 1.5 * (p75 - p25);
    upper = p75 + 1.5 * (p75 - p25);
  }
  // thread tid owns values tid, tid + 256, ... in every pass
  int cnt = 0;
  double s1 = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < L; i += 256) {
    bool k = false;
    if (i < n) {
      const float x = v[i];
      k = (double)x > lower && (double)x < upper;
      if (k) { ++cnt; s1 += (double)x; lo = fminf(lo, x); hi = fmaxf(hi, x); }
    }
    kp[i] = k ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  if ((tid & 63) == 0) { redi[tid >> 6] = cnt; redf[tid >> 6] = lo; redf[4 + (tid >> 6)] = hi; }
  const double total = ctts_block_sum_d(s1, red, tid);        // its barriers also publish redi / redf
  cnt = redi[0] + redi[1] + redi[2] + redi[3];
  const double mean = cnt > 0 ? total / (double)cnt : 0.0;
  double s2 = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double x = (double)v[i];
    if (x > lower && x < upper) { const double d = x - mean; s2 += d * d; }
  }
  const double ss = ctts_block_sum_d(s2, red, tid);
  if (tid == 0) {
    count[b] = cnt; sum[b] = total; m2[b] = ss;
    vmin[b] = fminf(fminf(redf[0], redf[1]), fminf(redf[2], redf[3]));
    vmax[b] = fmaxf(fmaxf(redf[4], redf[5]), fmaxf(redf[6], redf[7]));
  }
}

}  // namespace

extern "C" size_t ctts_trim_silence_workspace_bytes(int B, int N, int hop) {
  if (B <= 0 || N <= 0 || hop <= 0) return 0;
  return sizeof(float) * (size_t)B * (size_t)(1 + N / hop);
}

extern "C" int ctts_trim_silence(const float* wav, const int32_t* lens, float* workspace, int32_t* start, int32_t* end, int B, int N, float top_db,
                                 int frame_length, int hop, void* stream) {
  CTTS_REQUIRE(wav && lens && workspace && start && end && B > 0 && N > 0, "ctts_trim_silence: bad arguments");
  CTTS_REQUIRE(frame_length >= 2 && hop >= 1, "ctts_trim_silence: need frame_length >= 2 and hop >= 1 (got %d / %d)", frame_length, hop);
  CTTS_REQUIRE(top_db == top_db, "ctts_trim_silence: NaN top_db");
  CTTS_REQUIRE(B <= 65535, "ctts_trim_silence: at most 65535 utterances per call (got %d)", B);
  const int F = 1 + N / hop;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(frame_power_kernel, dim3((F + TRIM_FRAMES_PER_WG - 1) / TRIM_FRAMES_PER_WG, B), dim3(256), 0, st, wav, lens, workspace, N, F,
                     frame_length, hop);
  CTTS_CHECK_LAUNCH("ctts_trim_silence (frame power)");
  hipLaunchKernelGGL(trim_bounds_kernel, dim3(B), dim3(256), 0, st, workspace, lens, start, end, N, F, hop, top_db);
  CTTS_CHECK_LAUNCH("ctts_trim_silence");
  return 0;
}

extern "C" int ctts_attn_prior(const int32_t* src_lens, const int32_t* mel_lens, float* out, int B, int Ts, int Tm, int64_t stride_b, int64_t stride_s,
                               float scaling_factor, void* stream) {
  CTTS_REQUIRE(src_lens && mel_lens && out && B > 0 && Ts > 0 && Tm > 0, "ctts_attn_prior: bad arguments");
  CTTS_REQUIRE(scaling_factor > 0.f && scaling_factor < INFINITY, "ctts_attn_prior: scaling_factor must be positive and finite (got %g)",
               (double)scaling_factor);
  CTTS_REQUIRE(stride_s >= Tm && stride_b >= (int64_t)(Ts - 1) * stride_s + Tm, "ctts_attn_prior: rows of the output view overlap (strides %lld / %lld)",
               (long long)stride_b, (long long)stride_s);
  CTTS_REQUIRE(B <= 65535, "ctts_attn_prior: at most 65535 utterances per call (got %d)", B);
  hipLaunchKernelGGL(attn_prior_kernel, dim3(Ts, B), dim3(256), 0, (hipStream_t)stream, src_lens, mel_lens, out, Ts, Tm, (long)stride_b, (long)stride_s,
                     (double)scaling_factor);
  CTTS_CHECK_LAUNCH("ctts_attn_prior");
  return 0;
}

extern "C" int ctts_outlier_stats(const float* values, const int32_t* lens, uint8_t* keep, int32_t* count, double* sum, double* m2, float* vmin,
                                  float* vmax, int B, int L, void* stream) {
  CTTS_REQUIRE(values && lens && keep && count && sum && m2 && vmin && vmax && B > 0 && L > 0, "ctts_outlier_stats: bad arguments");
  CTTS_REQUIRE(L <= OUT_MAX, "ctts_outlier_stats: at most %d values per utterance are supported (got %d)", OUT_MAX, L);
  hipLaunchKernelGGL(outlier_stats_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, values, lens, keep, count, sum, m2, vmin, vmax, L);
  CTTS_CHECK_LAUNCH("ctts_outlier_stats");
  return 0;
}
