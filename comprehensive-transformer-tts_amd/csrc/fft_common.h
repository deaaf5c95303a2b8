// FFT routines shared by the audio kernels (mel.hip, griffinlim.hip, pitchtrack.hip, wavmetrics.hip, speaker.hip, preprocess.hip):
//   - the wave-private 512-point complex FFT (fp32, three radix-8 Stockham passes) behind every 1024-point real transform, with its
//     twiddle tables, the even/odd split and its inverse;
//   - the workgroup radix-2 FFT on double2 in LDS of the metric / feature kernels;
//   - the index arithmetic of reflect padding.
// The two FFTs are different algorithms in different precisions and stay two sets of routines.
#pragma once
#include "ctts_common.h"

// position u of a signal of L samples under reflect padding (F.pad(..., mode="reflect"), np.pad mode "reflect"): one reflection at
// either end, then clamped so that a signal shorter than the padding is still read in bounds.  I: int or long.
template <typename I>
__device__ __forceinline__ I ctts_reflect_index(I u, I L) {
  if (u < 0) u = -u;
  if (u >= L) u = 2 * (L - 1) - u;
  return min(max(u, (I)0), L - 1);
}

// ------------------------------------------------------------------------------------------------ complex helpers (fp32)
struct float2_ { float x, y; };
__device__ __forceinline__ float2_ cmul(float2_ a, float2_ b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ float2_ cadd(float2_ a, float2_ b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ float2_ csub(float2_ a, float2_ b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ void fft2(float2_& a, float2_& b) { const float2_ t = a; a = {t.x + b.x, t.y + b.y}; b = {t.x - b.x, t.y - b.y}; }
__device__ __forceinline__ float2_ mul_mi(float2_ a) { return {a.y, -a.x}; }       // * (-i)
__device__ __forceinline__ void fft4(float2_& v0, float2_& v1, float2_& v2, float2_& v3) {
  fft2(v0, v2); fft2(v1, v3); v3 = mul_mi(v3); fft2(v0, v1); fft2(v2, v3);         // -> X0 = v0, X2 = v1, X1 = v2, X3 = v3
}
// forward 8-point DFT in place; afterwards X[0..7] = v0, v4, v2, v6, v1, v5, v3, v7
__device__ __forceinline__ void fft8(float2_ (&v)[8]) {
  constexpr float h = 0.70710678118654752440f;
  fft2(v[0], v[4]); fft2(v[1], v[5]); fft2(v[2], v[6]); fft2(v[3], v[7]);
  v[5] = {(v[5].x + v[5].y) * h, (v[5].y - v[5].x) * h};        // * W8^1 = (1 - i)/sqrt2
  v[6] = mul_mi(v[6]);                                          // * W8^2 = -i
  v[7] = {(v[7].y - v[7].x) * h, -(v[7].x + v[7].y) * h};       // * W8^3 = (-1 - i)/sqrt2
  fft4(v[0], v[1], v[2], v[3]); fft4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ int brev3(int r) { return ((r & 1) << 2) | (r & 2) | (r >> 2); }

// ------------------------------------------------------------------------------------------------ the wave-private 512-point FFT
// One wave per frame, 8 points per lane, exchange through a scratch S of SCR complex slots (re | im interleaved) in LDS.
constexpr int SCR = 584;                   // per-wave FFT scratch: 512 complex + padding (pad32: index + index/32 + 8 * (index/64))
// twiddle tables, at the head of a workspace and of the LDS image alike (floats): [0, 1024) W512^m (cos, sin), m < 512 |
// [1024, 1540) W1024^k, k = 0..256 (cos, sin; k = 257 zero) | in LDS only: [1540, 1652) the 7 x 8 twiddles of FFT pass 1
constexpr int WS_W512 = 0, WS_W1024 = 1024, FFT_TW_FLOATS = 1540, FFT_TW1_FLOATS = 112;

// scratch slot of complex element i.  Every exchange pattern of the three passes must spread a 16-lane group over all 64 banks
// (8-byte accesses): consecutive i (pass reads, pass-2 writes), i = 8 * lane + r (pass-0 writes: + i/32 shifts every 4th lane by a
// bank pair) and i = 64 * (lane / 8) + (lane & 7) + 8 r (pass-1 writes: + 8 * (i/64) moves the second 8-lane run 20 banks away from
// the first; with i + i/32 alone the two runs overlapped in 12 of 16 banks - 2-way conflicts on all 8 writes of every lane).
__device__ __forceinline__ int pad32(int i) { return i + (i >> 5) + ((i >> 6) << 3); }

// The FFT scratch S is private to a wave: its 64 lanes exchange data through LDS in program order (LDS operations of one wave complete in
// order), so the passes need no workgroup barrier - only a fence that keeps hipcc from moving LDS accesses across the exchange points.
// (Round 2 had __syncthreads() there: five workgroup barriers per frame that made the four independent FFTs of a workgroup march in step.)
#define CTTS_WAVE_SYNC() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier()

// The tables in double precision, rounded once; every thread of ONE workgroup of `nthreads` calls this (the prepare kernels).
__device__ __forceinline__ void fft512_fill_tables(float* __restrict__ ws, int tid, int nthreads) {
  for (int m = tid; m < 512; m += nthreads) {
    double s, c; sincos(-2.0 * 3.14159265358979323846 * m / 512.0, &s, &c);
    ws[WS_W512 + 2 * m] = (float)c; ws[WS_W512 + 2 * m + 1] = (float)s;
  }
  for (int m = tid; m < 258; m += nthreads) {
    double s, c; sincos(-2.0 * 3.14159265358979323846 * m / 1024.0, &s, &c);
    ws[WS_W1024 + 2 * m] = m <= 256 ? (float)c : 0.f; ws[WS_W1024 + 2 * m + 1] = m <= 256 ? (float)s : 0.f;
  }
}

// Tables of a workspace -> the first FFT_TW_FLOATS + FFT_TW1_FLOATS floats of LDS, by a workgroup of 256 threads (no barrier here).
// Pass 1 needs only 8 distinct twiddles per r (jm = lane & 7); read from the W512 table they sit 64 r bytes apart - up to 8 lanes of
// a group on one bank.  A row of 8 consecutive entries per r, W512^(8 * jm * r) at [(r - 1) * 8 + jm], is conflict-free.
__device__ __forceinline__ void fft512_load_tables(float* lds, const float* __restrict__ ws, int tid) {
  for (int e = tid; e < FFT_TW_FLOATS; e += 256) lds[e] = ws[e];
  float* tw1 = lds + FFT_TW_FLOATS;
  if (tid < 56) { const int t = (tid & 7) * 8 * ((tid >> 3) + 1); tw1[2 * tid] = ws[2 * t]; tw1[2 * tid + 1] = ws[2 * t + 1]; }
}

// 512-point forward complex FFT of v[r] = z[lane + 64 r]; leaves Z[k] at S[pad32(k)].  tw512 / tw1: the LDS tables above.
// fft512 owns the fence between the wave's earlier READS of S and its first write: a caller may read S up to the call (the inverse
// loads v from S itself).  What the caller owns is the other direction: after reading the result it fences (or ends in a workgroup
// barrier) before anything but fft512 / merge_bins writes S again.
// mel_kernel (csrc/mel.hip) carries these passes written out, without the leading fence (it fences at the end of each frame) - see the
// comment there; a change to the passes is made here and there.
__device__ __forceinline__ void fft512(float2_ (&v)[8], float* S, const float* tw512, const float* tw1, int lane) {
  fft8(v);                                              // pass 0 (Ns = 1): no twiddles
  CTTS_WAVE_SYNC();                                     // every earlier read of S by this wave is done
#pragma unroll
  for (int r = 0; r < 8; ++r) { const int o = pad32(lane * 8 + r); S[2 * o] = v[brev3(r)].x; S[2 * o + 1] = v[brev3(r)].y; }
  CTTS_WAVE_SYNC();
#pragma unroll
  for (int pass = 1; pass < 3; ++pass) {                // pass 1 (Ns = 8) and pass 2 (Ns = 64)
    const int Ns = pass == 1 ? 8 : 64;
    const int jm = lane & (Ns - 1);
#pragma unroll
    for (int r = 0; r < 8; ++r) { const int o = pad32(lane + 64 * r); v[r] = {S[2 * o], S[2 * o + 1]}; }
#pragma unroll
    for (int r = 1; r < 8; ++r) {                       // W512^(jm * r * 64 / Ns)
      const float* tw = pass == 1 ? tw1 + 2 * ((r - 1) * 8 + jm) : tw512 + 2 * (jm * r);
      v[r] = cmul(v[r], float2_{tw[0], tw[1]});
    }
    fft8(v);
    CTTS_WAVE_SYNC();                                   // every lane of THIS wave has read its inputs
    const int idx = (lane / Ns) * Ns * 8 + jm;
#pragma unroll
    for (int r = 0; r < 8; ++r) { const int o = pad32(idx + r * Ns); S[2 * o] = v[brev3(r)].x; S[2 * o + 1] = v[brev3(r)].y; }
    CTTS_WAVE_SYNC();
  }
}

// even / odd split after fft512 of z[n] = x[2n] + i x[2n+1]: the 1024-point spectrum of the real x at bins k = lane + 64 m (m < 4),
// their mirrors 512 - k, and bin 256 (same value in every lane)
__device__ __forceinline__ void split_bins(const float* S, const float* tw1024, int lane, float2_ (&xk)[4], float2_ (&xm)[4], float2_& x256) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int k = lane + 64 * m;
    const int o1 = pad32(k), o2 = pad32((512 - k) & 511);
    const float a = S[2 * o1], b = S[2 * o1 + 1], c = S[2 * o2], d = S[2 * o2 + 1];
    const float er = 0.5f * (a + c), ei = 0.5f * (b - d), orr = 0.5f * (b + d), oi = -0.5f * (a - c);
    const float wr = tw1024[2 * k], wi = tw1024[2 * k + 1];
    const float tr = wr * orr - wi * oi, ti = wr * oi + wi * orr;
    xk[m] = {er + tr, ei + ti};                         // X[k]       = E + W^k O
    xm[m] = {er - tr, ti - ei};                         // X[512 - k] = conj(E - W^k O)
  }
  const int o = pad32(256);
  x256 = {S[2 * o], -S[2 * o + 1]};                     // X[256] = conj(Z[256])
}

// inverse of split_bins: writes conj(Z') for the half spectrum X' (imaginary parts of bins 0 and 512 dropped) so that the forward FFT
// of S gives 512 conj(z'), z'[m] = x[2m] + i x[2m+1] of x = irfft(X')
__device__ __forceinline__ void merge_bins(float* S, const float* tw1024, int lane, const float2_ (&xk)[4], const float2_ (&xm)[4], float2_ x256) {
  CTTS_WAVE_SYNC();                                     // every lane has read S (split_bins)
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int k = lane + 64 * m;
    float2_ a = xk[m], c = xm[m];
    if (k == 0) { a.y = 0.f; c.y = 0.f; }
    const float er = 0.5f * (a.x + c.x), ei = 0.5f * (a.y - c.y);       // E = (X[k] + conj X[512-k]) / 2
    const float dr = 0.5f * (a.x - c.x), di = 0.5f * (a.y + c.y);       // D = (X[k] - conj X[512-k]) / 2,  O = D conj(W^k)
    const float wr = tw1024[2 * k], wi = tw1024[2 * k + 1];
    const float orr = dr * wr + di * wi, oi = di * wr - dr * wi;
    const int o1 = pad32(k);
    S[2 * o1] = er - oi; S[2 * o1 + 1] = -(ei + orr);   // conj(Z[k]),       Z[k] = E + i O
    if (k) {
      const int o2 = pad32(512 - k);
      S[2 * o2] = er + oi; S[2 * o2 + 1] = ei - orr;    // conj(Z[512 - k]), Z[512-k] = conj(E) + i conj(O)
    }
  }
  if (lane == 0) { const int o = pad32(256); S[2 * o] = x256.x; S[2 * o + 1] = x256.y; }     // conj(Z[256]) = X[256]
  CTTS_WAVE_SYNC();
}

// ------------------------------------------------------------------------------------------------ the workgroup FFT on double2 in LDS
// Radix 2, decimation in time, NFFT points by a workgroup of THREADS: the caller stores sample n at a[ctts_dfft_slot<NFFT>(n)], fills
// tw[NFFT / 2] once, puts a __syncthreads() behind both and runs the log2(NFFT) passes; the spectrum is then in natural order in a[],
// visible to every thread.
template <int NFFT>
struct ctts_log2 {
  static constexpr int value = 1 + ctts_log2<NFFT / 2>::value;
};
template <>
struct ctts_log2<1> {
  static constexpr int value = 0;
};

template <int NFFT>
__device__ __forceinline__ int ctts_dfft_slot(int n) { return (int)(__brev((unsigned)n) >> (32 - ctts_log2<NFFT>::value)); }

// tw[k] = W_NFFT^k = exp(-2 pi i k / NFFT); the argument of sincospi is exact
template <int NFFT, int THREADS>
__device__ __forceinline__ void ctts_dfft_fill_twiddles(double2* tw, int tid) {
  for (int k = tid; k < NFFT / 2; k += THREADS) {
    double s, c;
    sincospi(-2.0 * (double)k / (double)NFFT, &s, &c);
    tw[k] = make_double2(c, s);
  }
}

// pass s of ctts_log2<NFFT>::value, s = 0 first; ends in a workgroup barrier.  The loop over s is the caller's, which decides whether it
// is unrolled: frame_spectrum (three sizes, two epilogues) keeps it rolled, fbank_kernel leaves it to the compiler.
template <int NFFT, int THREADS>
__device__ __forceinline__ void ctts_dfft_pass(double2* a, const double2* tw, int s, int tid) {
  constexpr int LOG = ctts_log2<NFFT>::value;
  const int half = 1 << s;
  for (int t = tid; t < NFFT / 2; t += THREADS) {
    const int pos = t & (half - 1);
    const int i = 2 * t - pos, j = i + half;           // = ((t >> s) << (s + 1)) + pos
    const double2 w = tw[pos << (LOG - 1 - s)];
    const double2 u = a[i], q = a[j];
    // the products and sums exactly in this form: which of them contract into fused multiply-adds decides the bits
    const double vr = q.x * w.x - q.y * w.y, vi = q.x * w.y + q.y * w.x;
    a[i] = make_double2(u.x + vr, u.y + vi);
    a[j] = make_double2(u.x - vr, u.y - vi);
  }
  __syncthreads();
}
