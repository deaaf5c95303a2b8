// Pitch targets on the device (include/ctts.h "Pitch targets on the device"): the training inputs the reference
// makes offline with parselmouth + pycwt (utils/pitch_tools.py:85-255, preprocessor.py:612-618) from the waveform alone.
//
// pitch_track_kernel - one wave per frame, four frames per wave, 16 per workgroup.  A frame's 1024 windowed samples go through a 2048-point
//   zero-padded real FFT = one 1024-point complex FFT (z[n] = x[2n] + i x[2n+1], five radix-4 Stockham passes, 16 points per lane, exchange
//   through the wave's own LDS scratch, no workgroup barrier: see CTTS_WAVE_SYNC in fft_common.h) + the even/odd split; the power spectrum is
//   real and even, so the way back is the SAME transform (its real part is 2048 r(tau)).  Normalisation by the window's autocorrelation,
//   the candidate search and the octave-cost argmax stay in LDS and registers: HBM traffic = the samples in, 8 bytes per frame out.
// f0_targets_kernel - one workgroup per utterance: nearest voiced neighbour on both sides (chunked scan), continuous log-F0, mean / std in
//   double, and the Mexican-hat CWT as ONE forward radix-2 FFT of the utterance's own power-of-two length plus FIVE inverse ones (the
//   wavelet's spectrum is real, so two scales ride in the real and imaginary part of one inverse transform), all in LDS.
// No float atomics, no inter-workgroup waits, every loop statically bounded: results are bit-reproducible and batch-independent.
#include "ctts_common.h"
#include "fft_common.h"
#include <math.h>

namespace {

constexpr int FRAME = 1024, NZ = 1024, NLAG = 512;          // samples per frame, complex FFT length, lags kept
// workspace (floats): W1024^m (cos, sin) m < 1024 | W2048^k (cos, sin) k < 512 | periodic hann [1024] | r_w(tau) / r_w(0), tau < 512
constexpr int WS_TW = 0, WS_TW2 = 2048, WS_WIN = 3072, WS_RWN = 4096, WS_FLOATS = 4608;
constexpr int PW = 1028;                                     // per-wave power spectrum P[0..1024]
constexpr int FRAMES_PER_WAVE = 4, FRAMES_PER_WG = 16;
constexpr int PEAK_SLICES = 32;                             // the utterance peak is reduced in 32 slices per utterance

// In-place forward 1024-point complex FFT of the wave's scratch S (natural order in and out): Stockham radix 4, butterfly j = lane + 64 q
// reads S[j + 256 r], multiplies by W1024^(r k 256 / Ns) (k = j mod Ns) and writes S[4 (j - k) + k + r Ns].  Every lane holds all 16 of its
// inputs before any lane writes (the wave runs in lockstep between the two fences), which is what makes the in-place update safe.
__device__ __forceinline__ void fft1024(float* __restrict__ S, const float* __restrict__ tw, int lane) {
#pragma unroll
  for (int pass = 0; pass < 5; ++pass) {
    const int Ns = 1 << (2 * pass);
    float2_ u[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q;
#pragma unroll
      for (int r = 0; r < 4; ++r) u[q][r] = {S[2 * (j + 256 * r)], S[2 * (j + 256 * r) + 1]};
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q, k = j & (Ns - 1);
      if (pass > 0) {
        const int m = k * (256 / Ns);
#pragma unroll
        for (int r = 1; r < 4; ++r) u[q][r] = cmul(u[q][r], float2_{tw[2 * (r * m)], tw[2 * (r * m) + 1]});
      }
      const float2_ t0 = cadd(u[q][0], u[q][2]), t1 = csub(u[q][0], u[q][2]), t2 = cadd(u[q][1], u[q][3]), d = csub(u[q][1], u[q][3]);
      const float2_ t3 = {d.y, -d.x};                                  // * (-i)
      u[q][0] = cadd(t0, t2); u[q][1] = cadd(t1, t3); u[q][2] = csub(t0, t2); u[q][3] = csub(t1, t3);
    }
    CTTS_WAVE_SYNC();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q, k = j & (Ns - 1), j0 = ((j - k) << 2) + k;
#pragma unroll
      for (int r = 0; r < 4; ++r) { S[2 * (j0 + r * Ns)] = u[q][r].x; S[2 * (j0 + r * Ns) + 1] = u[q][r].y; }
    }
    CTTS_WAVE_SYNC();
  }
}

// bins k and 1024 - k of the 2048-point transform of the real sequence packed into S: X[k] = E + W2048^k O, X[1024 - k] = conj(E - W2048^k O)
__device__ __forceinline__ void split_pair(const float* __restrict__ S, const float* __restrict__ tw2, int k, float2_& xa, float2_& xb) {
  const int km = (NZ - k) & (NZ - 1);
  const float a = S[2 * k], b = S[2 * k + 1], c = S[2 * km], d = S[2 * km + 1];
  const float2_ E = {0.5f * (a + c), 0.5f * (b - d)}, O = {0.5f * (b + d), -0.5f * (a - c)};
  const float2_ t = cmul(float2_{tw2[2 * k], tw2[2 * k + 1]}, O);
  xa = cadd(E, t);
  xb = csub(E, t);                                                // conjugate not taken: only |.|^2 or the real part is used
}

// peak |x| of slice blockIdx.x (of PEAK_SLICES) of utterance blockIdx.y -> peak[b][slice]; the tracker takes the maximum of the slices
// (a maximum does not depend on the order: no atomics, no second launch)
__global__ __launch_bounds__(256) void utterance_peak_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, float* __restrict__ peak,
                                                              int N) {
  __shared__ float red[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int len = lens ? min(max(lens[b], 0), N) : N;
  const int chunk = (N + PEAK_SLICES - 1) / PEAK_SLICES;
  const int i0 = min((int)blockIdx.x * chunk, len), i1 = min(i0 + chunk, len);
  const float* x = wav + (long)b * N;
  float m = 0.f;
  for (int i = i0 + tid; i < i1; i += 256) m = fmaxf(m, fabsf(x[i]));
  m = ctts_wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) peak[b * PEAK_SLICES + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void pitch_track_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, const float* __restrict__ ws,
                                                           const float* __restrict__ peak, float* __restrict__ f0_out, float* __restrict__ st_out,
                                                           int B, int N, int F, int hop, int lag_lo, int lag_hi, float sr, float f0_min,
                                                           float vthr, float sthr) {
  __shared__ __attribute__((aligned(16))) float lds[WS_WIN + NLAG + 4 * (2 * NZ + PW)];
  float* tw = lds;                                       // 2048
  float* tw2 = lds + WS_TW2;                             // 1024
  float* rwn = lds + WS_WIN;                             // 512
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* S = lds + WS_WIN + NLAG + wave * (2 * NZ + PW);
  float* P = S + 2 * NZ;
  for (int e = tid; e < WS_WIN; e += 256) lds[e] = ws[e];
  for (int e = tid; e < NLAG; e += 256) rwn[e] = ws[WS_RWN + e];
  float win[16];
#pragma unroll
  for (int m = 0; m < 8; ++m) { win[2 * m] = ws[WS_WIN + 2 * (lane + 64 * m)]; win[2 * m + 1] = ws[WS_WIN + 2 * (lane + 64 * m) + 1]; }
  __syncthreads();
  const long total = (long)B * F;
  for (int ff = 0; ff < FRAMES_PER_WAVE; ++ff) {
    const long g = (long)blockIdx.x * FRAMES_PER_WG + wave * FRAMES_PER_WAVE + ff;    // wave-uniform
    if (g >= total) break;
    const int b = (int)(g / F), t = (int)(g - (long)b * F);
    const int len = lens ? min(max(lens[b], 0), N) : N;
    float f0v = 0.f, stv = 0.f;
    if (t < 1 + len / hop) {
      const float* x = wav + (long)b * N;
      const long base = (long)t * hop - FRAME / 2;
      // ---- load: samples 2n, 2n + 1 for n = lane + 64 m; outside [0, len) reads as zero
      float xs[16], sum = 0.f, amax = 0.f;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const long i = base + 2 * (lane + 64 * m) + h;
          const float v = (i >= 0 && i < len) ? x[i] : 0.f;
          xs[2 * m + h] = v; sum += v; amax = fmaxf(amax, fabsf(v));
        }
      }
      const float mean = ctts_wave_sum(sum) * (1.0f / FRAME);
      amax = ctts_wave_max(amax);
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int n = lane + 64 * m;
        S[2 * n] = (xs[2 * m] - mean) * win[2 * m]; S[2 * n + 1] = (xs[2 * m + 1] - mean) * win[2 * m + 1];
        S[2 * (n + 512)] = 0.f; S[2 * (n + 512) + 1] = 0.f;      // the zero padding to 2048 samples
      }
      CTTS_WAVE_SYNC();
      fft1024(S, tw, lane);
      // ---- power spectrum P[0..1024] (P[2048 - k] = P[k])
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int k = lane + 64 * m;
        float2_ xa, xb; split_pair(S, tw2, k, xa, xb);
        P[k] = xa.x * xa.x + xa.y * xa.y;
        P[NZ - k] = xb.x * xb.x + xb.y * xb.y;
      }
      if (lane == 0) { const float a = S[2 * 512], c = S[2 * 512 + 1]; P[512] = a * a + c * c; }    // E, O real and W2048^512 = -i: |X[512]| = |Z[512]|
      CTTS_WAVE_SYNC();
      // ---- back: p[n] = P[n] (n <= 1024) or P[2048 - n], packed z[m] = p[2m] + i p[2m + 1]
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = lane + 64 * q, n0 = 2 * m, n1 = 2 * m + 1;
        S[2 * m] = P[n0 <= 1024 ? n0 : 2048 - n0]; S[2 * m + 1] = P[n1 <= 1024 ? n1 : 2048 - n1];
      }
      CTTS_WAVE_SYNC();
      fft1024(S, tw, lane);
      float r[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) { float2_ xa, xb; split_pair(S, tw2, lane + 64 * m, xa, xb); r[m] = xa.x; }   // 2048 r(tau), tau = lane + 64 m
      CTTS_WAVE_SYNC();
      const float r0 = __shfl(r[0], 0, 64);
      if (r0 > 0.f && r0 < INFINITY) {
        float* rn = S;                                   // rn[tau], tau < 512
#pragma unroll
        for (int m = 0; m < 8; ++m) { r[m] = (r[m] / r0) / rwn[lane + 64 * m]; rn[lane + 64 * m] = r[m]; }
        CTTS_WAVE_SYNC();
        float best_cost = -INFINITY, best_lag = 0.f, best_h = 0.f;
        int best_tau = 0x7fffffff;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const int tau = lane + 64 * m;
          if (tau >= lag_lo && tau <= lag_hi) {          // lag_lo >= 2, lag_hi + 1 < 512: both neighbours exist
            const float a = rn[tau - 1], bq = r[m], c = rn[tau + 1];
            if (bq > a && bq >= c) {
              const float den = (a - bq) + (c - bq);     // < 0
              const float dl = 0.5f * (a - c) / den;
              const float lag = (float)tau + dl, h = bq - 0.25f * (a - c) * dl;
              const float cost = h - 0.01f * log2f(f0_min * lag / sr);
              if (cost > best_cost) { best_cost = cost; best_lag = lag; best_h = h; best_tau = tau; }     // ascending tau: ties keep the smaller lag
            }
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float oc = __shfl_xor(best_cost, o, 64), ol = __shfl_xor(best_lag, o, 64), oh = __shfl_xor(best_h, o, 64);
          const int ot = __shfl_xor(best_tau, o, 64);
          if (oc > best_cost || (oc == best_cost && ot < best_tau)) { best_cost = oc; best_lag = ol; best_h = oh; best_tau = ot; }
        }
        if (best_tau != 0x7fffffff) {
          stv = best_h;
          const float upeak = ctts_wave_max(lane < PEAK_SLICES ? peak[b * PEAK_SLICES + lane] : 0.f);
          if (best_h >= vthr && amax >= sthr * upeak) f0v = sr / best_lag;
        }
      }
      CTTS_WAVE_SYNC();                                    // the scratch is reused by the wave's next frame
    }
    if (lane == 0) { f0_out[g] = f0v; st_out[g] = stv; }
  }
}

__global__ __launch_bounds__(256) void pitch_track_prepare_kernel(float* __restrict__ ws) {
  __shared__ double w[FRAME];
  const int tid = threadIdx.x;
  const double pi = 3.14159265358979323846;
  for (int m = tid; m < 1024; m += 256) {
    double s, c; sincos(-2.0 * pi * m / 1024.0, &s, &c);
    ws[WS_TW + 2 * m] = (float)c; ws[WS_TW + 2 * m + 1] = (float)s;
    w[m] = 0.5 - 0.5 * cos(2.0 * pi * m / 1024.0);
    ws[WS_WIN + m] = (float)w[m];
  }
  for (int m = tid; m < 512; m += 256) {
    double s, c; sincos(-2.0 * pi * m / 2048.0, &s, &c);
    ws[WS_TW2 + 2 * m] = (float)c; ws[WS_TW2 + 2 * m + 1] = (float)s;
  }
  __syncthreads();
  double r0 = 0.0;
  for (int n = 0; n < FRAME; ++n) r0 += w[n] * w[n];
  for (int tau = tid; tau < NLAG; tau += 256) {
    double r = 0.0;
    for (int n = 0; n + tau < FRAME; ++n) r += w[n] * w[n + tau];
    ws[WS_RWN + tau] = (float)(r / r0);
  }
}

// ------------------------------------------------------------------------------------------------------------------ target chain
constexpr int TMAX = 4096, NSCALE = 10;
// dynamic LDS (floats): val [TMAX] | bufA, bufB, bufX [2 TMAX] each | twiddles [TMAX] (M / 2 complex) | int chunk summaries [512]
constexpr int L_VAL = 0, L_A = TMAX, L_B = 3 * TMAX, L_X = 5 * TMAX, L_TW = 7 * TMAX, L_CH = 8 * TMAX, L_FLOATS = 8 * TMAX + 512;

// Stockham radix-2 FFT of M = 2^logM points by the whole workgroup, ping-pong between `in` and `out`; returns where the result lies
__device__ __forceinline__ float* block_fft(float* in, float* out, const float* __restrict__ tw, int M, int logM, bool inverse, int tid) {
  const int half = M >> 1;
  for (int s = 0; s < logM; ++s) {                       // logM <= 12
    const int Ns = 1 << s;
    for (int j = tid; j < half; j += 256) {
      const int k = j & (Ns - 1), ti = k * (half >> s);
      const float2_ a = {in[2 * j], in[2 * j + 1]};
      float2_ w = {tw[2 * ti], tw[2 * ti + 1]};
      if (inverse) w.y = -w.y;
      const float2_ bb = cmul(float2_{in[2 * (j + half)], in[2 * (j + half) + 1]}, w);
      const int j0 = ((j - k) << 1) + k;
      out[2 * j0] = a.x + bb.x; out[2 * j0 + 1] = a.y + bb.y;
      out[2 * (j0 + Ns)] = a.x - bb.x; out[2 * (j0 + Ns) + 1] = a.y - bb.y;
    }
    __syncthreads();
    float* t = in; in = out; out = t;
  }
  return in;
}

// log2 / log through double: correctly rounded float results (the contour feeds a mean, a std and a division by that std)
__device__ __forceinline__ float lg2(float x) { return (float)log2((double)x); }

// MODE 0: uv, cont_lf0, mean_std, cwt_spec, valid.   MODE 1: out0 = norm_interp_f0 (log2, np.interp over the unvoiced frames), uv.
template <int MODE>
__global__ __launch_bounds__(256) void f0_targets_kernel(const float* __restrict__ f0, const int32_t* __restrict__ frames, float* __restrict__ uv,
                                                          float* __restrict__ out0, float* __restrict__ mean_std, float* __restrict__ cwt,
                                                          int32_t* __restrict__ valid, int F, float eps) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ double red[4];
  __shared__ float redf[8];
  float* val = sm + L_VAL;
  int* pv = reinterpret_cast<int*>(sm + L_A);            // nearest voiced frame at or before t (-1: none) - bufA is free until the FFTs
  int* nx = pv + TMAX;                                   // nearest voiced frame at or after t (TMAX: none)
  int* ch_last = reinterpret_cast<int*>(sm + L_CH);
  int* ch_first = ch_last + 256;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(frames[b], 0), F);
  const float* fb = f0 + (long)b * F;
  float* uvb = uv + (long)b * F;
  float* ob = out0 + (long)b * F;
  float* cb = MODE == 0 ? cwt + (long)b * F * NSCALE : nullptr;
  // ---- padding frames are zero in every output; thread tid owns frames tid, tid + 256, ... in every pass over global memory
  for (int t = n + tid; t < F; t += 256) {
    uvb[t] = 0.f; ob[t] = 0.f;
    if (MODE == 0) {
#pragma unroll
      for (int j = 0; j < NSCALE; ++j) cb[(long)t * NSCALE + j] = 0.f;
    }
  }
  for (int t = tid; t < n; t += 256) val[t] = fb[t];
  __syncthreads();
  // ---- nearest voiced neighbours: thread tid scans frames [tid CH, (tid + 1) CH), the 256 chunk summaries are combined by every thread
  const int CH = (n + 255) / 256;                        // <= 16
  const int c0 = min(tid * CH, n), c1 = min(c0 + CH, n);
  int last = -1, first = TMAX;
  for (int t = c0; t < c1; ++t) if (val[t] != 0.f) { last = t; if (first == TMAX) first = t; }
  ch_last[tid] = last; ch_first[tid] = first;
  __syncthreads();
  int carry_prev = -1, carry_next = TMAX, first_v = TMAX, last_v = -1;
  for (int i = 0; i < 256; ++i) {
    const int l = ch_last[i], f = ch_first[i];
    if (i < tid) carry_prev = max(carry_prev, l);
    if (i > tid) carry_next = min(carry_next, f);
    last_v = max(last_v, l); first_v = min(first_v, f);
  }
  { int p = carry_prev; for (int t = c0; t < c1; ++t) { if (val[t] != 0.f) p = t; pv[t] = p; } }
  { int q = carry_next; for (int t = c1 - 1; t >= c0; --t) { if (val[t] != 0.f) q = t; nx[t] = q; } }
  __syncthreads();
  const bool any_voiced = last_v >= 0;
  if (MODE == 1) {
    // norm_interp_f0: y = log2(f0 + eps) at voiced frames; unvoiced ones by np.interp (slope * (x - x_lo) + y_lo), edge values held
    for (int t = tid; t < n; t += 256) {
      const float v = val[t];
      float y = 0.f;
      if (any_voiced) {
        if (v != 0.f) y = lg2(v + eps);
        else {
          const int p = pv[t], q = nx[t];
          if (p < 0) y = lg2(val[q] + eps);
          else if (q >= TMAX) y = lg2(val[p] + eps);
          else { const float yp = lg2(val[p] + eps), yq = lg2(val[q] + eps); y = (yq - yp) / (float)(q - p) * (float)(t - p) + yp; }
        }
      }
      ob[t] = y; uvb[t] = v == 0.f ? 1.f : 0.f;
    }
    return;
  }
  // ---- continuous log-F0.  convert_continuos_f0 finds the start by VALUE (first index holding the first voiced value) and the end
  // likewise (last index holding the last voiced value): every earlier / later frame is 0 and the value is not, so these ARE first_v / last_v.
  float lf[TMAX / 256];
  double s1 = 0.0;
  float vmin = INFINITY, vmax = -INFINITY;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < TMAX / 256; ++i) {
    const int t = tid + 256 * i;
    lf[i] = 0.f;
    if (t < n && any_voiced) {
      const float v = val[t];
      float y;
      if (t <= first_v) y = val[first_v];
      else if (t >= last_v) y = val[last_v];
      else if (v != 0.f) y = v;
      else { const int p = pv[t], q = nx[t]; const float yp = val[p], yq = val[q]; y = (yq - yp) / (float)(q - p) * (float)(t - p) + yp; }
      lf[i] = (float)log((double)y);              // correctly rounded: n <= 4096 values per utterance, the cost is nothing
      s1 += (double)lf[i];
      vmin = fminf(vmin, lf[i]); vmax = fmaxf(vmax, lf[i]);
      bad |= !(fabsf(lf[i]) < INFINITY);
    }
  }
  const double mean = ctts_block_sum_d(s1, red, tid) / (double)max(n, 1);
  double s2 = 0.0;
#pragma unroll
  for (int i = 0; i < TMAX / 256; ++i) { const int t = tid + 256 * i; if (t < n) { const double d = (double)lf[i] - mean; s2 += d * d; } }
  const double var = ctts_block_sum_d(s2, red, tid) / (double)max(n, 1);
  // ---- validity, decided without leaving the device: no voiced frame, a constant track (std == 0 exactly when max == min) or a
  // non-finite value (f0 < 0, Inf, NaN) give valid = 0 and all-zero rows
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { vmin = fminf(vmin, __shfl_xor(vmin, o, 64)); vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64)); }
  __syncthreads();
  if ((tid & 63) == 0) { redf[tid >> 6] = vmin; redf[4 + (tid >> 6)] = vmax; }
  __syncthreads();
  const float gmin = fminf(fminf(redf[0], redf[1]), fminf(redf[2], redf[3])), gmax = fmaxf(fmaxf(redf[4], redf[5]), fmaxf(redf[6], redf[7]));
  const float meanf = (float)mean, stdf = (float)sqrt(var);
  const int any_bad = __syncthreads_or((int)bad);
  // n == 2 has M = 2, where pycwt's w_1 = 2 pi fftfreq(2, dt)[1] is the Nyquist bin and negative: its sqrt(s_j w_1 M) is NaN for every
  // scale, a non-finite output like any other (the closed form sqrt(4 pi 2^j) below holds for M >= 4 only)
  bool ok = any_voiced && !any_bad && n > 2 && gmax > gmin && fabsf(meanf) < INFINITY && stdf > 0.f && stdf < INFINITY;     // block-uniform
  if (ok) {
    int logM = 0;
    while ((1 << logM) < n) ++logM;                      // n <= 4096: at most 12 steps
    const int M = 1 << logM;
    float* A = sm + L_A; float* Bf = sm + L_B; float* X = sm + L_X; float* tw = sm + L_TW;
    for (int k = tid; k < (M >> 1); k += 256) {
      double s, c; sincos(-2.0 * 3.14159265358979323846 * (double)k / (double)M, &s, &c);
      tw[2 * k] = (float)c; tw[2 * k + 1] = (float)s;
    }
#pragma unroll
    for (int i = 0; i < TMAX / 256; ++i) {
      const int t = tid + 256 * i;
      if (t < M) { A[2 * t] = t < n ? (lf[i] - meanf) / stdf : 0.f; A[2 * t + 1] = 0.f; }
      if (t < n) { ob[t] = lf[i]; uvb[t] = val[t] == 0.f ? 1.f : 0.f; }
    }
    __syncthreads();
    float* res = block_fft(A, Bf, tw, M, logM, false, tid);
    for (int k = tid; k < 2 * M; k += 256) X[k] = res[k];
    __syncthreads();
    const float invM = 1.0f / (float)M;
    bool nonfinite = false;
    for (int p = 0; p < NSCALE / 2; ++p) {
      // scales s_j = 0.01 2^j, j = 2p and 2p + 1: s_j w_k = 4 pi 2^j k' / M and sqrt(s_j w_1 M) = sqrt(4 pi 2^j), whatever M is
      const float ca = 12.566370614359172f * (float)(1 << (2 * p)), cbb = 2.0f * ca;
      const float na = sqrtf(ca) * 0.8673250705840776f, nb = sqrtf(cbb) * 0.8673250705840776f;       // / sqrt(Gamma(2.5))
      for (int k = tid; k < M; k += 256) {
        const float fr = (float)(k <= (M >> 1) ? k : M - k) * invM;                                   // |fftfreq| (the wavelet's spectrum is even)
        const float fa = ca * fr, fb = cbb * fr;
        const float ga = na * (fa * fa) * expf(-0.5f * (fa * fa)), gb = nb * (fb * fb) * expf(-0.5f * (fb * fb));
        const float xr = X[2 * k], xi = X[2 * k + 1];
        A[2 * k] = xr * ga - xi * gb; A[2 * k + 1] = xr * gb + xi * ga;                               // X (ga + i gb): two real outputs per inverse
      }
      __syncthreads();
      res = block_fft(A, Bf, tw, M, logM, true, tid);
      for (int t = tid; t < n; t += 256) {
        const float wa = res[2 * t] * invM, wb = res[2 * t + 1] * invM;
        cb[(long)t * NSCALE + 2 * p] = wa; cb[(long)t * NSCALE + 2 * p + 1] = wb;
        nonfinite |= !(fabsf(wa) < INFINITY) || !(fabsf(wb) < INFINITY);
      }
      __syncthreads();
    }
    ok = !__syncthreads_or((int)nonfinite);
  }
  if (!ok) {
    for (int t = tid; t < n; t += 256) {
      uvb[t] = 0.f; ob[t] = 0.f;
#pragma unroll
      for (int j = 0; j < NSCALE; ++j) cb[(long)t * NSCALE + j] = 0.f;
    }
  }
  if (tid == 0) { mean_std[2 * b] = ok ? meanf : 0.f; mean_std[2 * b + 1] = ok ? stdf : 0.f; valid[b] = ok ? 1 : 0; }
}

}  // namespace

extern "C" size_t ctts_pitch_track_workspace_bytes(void) { return sizeof(float) * (size_t)WS_FLOATS; }

extern "C" int ctts_pitch_track_prepare(float* workspace, void* stream) {
  CTTS_REQUIRE(workspace, "ctts_pitch_track_prepare: null pointer");
  hipLaunchKernelGGL(pitch_track_prepare_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace);
  CTTS_CHECK_LAUNCH("ctts_pitch_track_prepare");
  return 0;
}

extern "C" int ctts_pitch_track(const float* wav, const int32_t* lens, const float* workspace, float* peak, float* f0, float* strength, int B, int N,
                                int sr, int hop, float f0_min, float f0_max, float voicing_threshold, float silence_threshold, void* stream) {
  CTTS_REQUIRE(wav && workspace && peak && f0 && strength && B > 0 && N > 0, "ctts_pitch_track: bad arguments");
  CTTS_REQUIRE(sr > 0 && hop > 0, "ctts_pitch_track: sr and hop must be positive (got %d / %d)", sr, hop);
  CTTS_REQUIRE(f0_min > 0.f && f0_max > f0_min && f0_max < INFINITY, "ctts_pitch_track: need 0 < f0_min < f0_max (got %g / %g)", (double)f0_min, (double)f0_max);
  CTTS_REQUIRE(voicing_threshold == voicing_threshold && silence_threshold == silence_threshold, "ctts_pitch_track: NaN threshold");
  const double lo_d = floor((double)sr / (double)f0_max), hi_d = ceil((double)sr / (double)f0_min);
  CTTS_REQUIRE(lo_d >= 2.0 && hi_d + 1.0 < (double)NLAG,
               "ctts_pitch_track: lag range [%.0f, %.0f] (sr %d, f0 %g .. %g Hz) does not fit the 1024-sample frame: need 2 <= lags and lag + 1 < 512",
               lo_d, hi_d, sr, (double)f0_min, (double)f0_max);
  const int F = 1 + N / hop;
  const long total = (long)B * F;
  CTTS_REQUIRE(total <= 0x7fffffffL && B <= 65535, "ctts_pitch_track: too many frames or utterances");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(utterance_peak_kernel, dim3(PEAK_SLICES, B), dim3(256), 0, st, wav, lens, peak, N);
  CTTS_CHECK_LAUNCH("ctts_pitch_track (peak)");
  const int grid = (int)((total + FRAMES_PER_WG - 1) / FRAMES_PER_WG);
  hipLaunchKernelGGL(pitch_track_kernel, dim3(grid), dim3(256), 0, st, wav, lens, workspace, peak, f0, strength, B, N, F, hop, (int)lo_d, (int)hi_d,
                     (float)sr, f0_min, voicing_threshold, silence_threshold);
  CTTS_CHECK_LAUNCH("ctts_pitch_track");
  return 0;
}

static int f0_targets_check(const char* what, const void* f0, const void* frames, int B, int F) {
  CTTS_REQUIRE(f0 && frames && B > 0 && F > 0, "%s: bad arguments", what);
  CTTS_REQUIRE(F <= TMAX, "%s: at most %d frames per utterance are supported (got %d)", what, TMAX, F);
  return 0;
}

extern "C" int ctts_f0_targets(const float* f0, const int32_t* frames, float* uv, float* cont_lf0, float* mean_std, float* cwt_spec, int32_t* valid,
                               int B, int F, void* stream) {
  if (int e = f0_targets_check("ctts_f0_targets", f0, frames, B, F)) return e;
  CTTS_REQUIRE(uv && cont_lf0 && mean_std && cwt_spec && valid, "ctts_f0_targets: null output");
  const size_t lds_bytes = sizeof(float) * (size_t)L_FLOATS;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(f0_targets_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  hipLaunchKernelGGL(f0_targets_kernel<0>, dim3(B), dim3(256), lds_bytes, (hipStream_t)stream, f0, frames, uv, cont_lf0, mean_std, cwt_spec, valid, F, 0.f);
  CTTS_CHECK_LAUNCH("ctts_f0_targets");
  return 0;
}

extern "C" int ctts_norm_interp_f0(const float* f0, const int32_t* frames, float* f0_norm, float* uv, int B, int F, float eps, void* stream) {
  if (int e = f0_targets_check("ctts_norm_interp_f0", f0, frames, B, F)) return e;
  CTTS_REQUIRE(f0_norm && uv, "ctts_norm_interp_f0: null output");
  CTTS_REQUIRE(eps >= 0.f && eps < INFINITY, "ctts_norm_interp_f0: eps must be finite and >= 0");
  const size_t lds_bytes = sizeof(float) * (size_t)L_FLOATS;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(f0_targets_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  hipLaunchKernelGGL(f0_targets_kernel<1>, dim3(B), dim3(256), lds_bytes, (hipStream_t)stream, f0, frames, uv, f0_norm, nullptr, nullptr, nullptr, F, eps);
  CTTS_CHECK_LAUNCH("ctts_norm_interp_f0");
  return 0;
}
