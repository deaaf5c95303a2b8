// Griffin-Lim on a real FFT (reference audio/stft.py:22-134 STFT.transform / inverse, audio/audio_processing.py:7-82 window_sumsquare /
// griffin_lim).  n_fft = 1024, hop = 256 only.
//
// The reference runs both directions as conv1d / conv_transpose1d against a dense [1026 x 1024] windowed basis (4.2 MFLOP per frame and
// iteration).  Here each frame is one wave: a 1024-point real FFT = a 512-point complex FFT (z[m] = x[2m] + i x[2m+1], three radix-8
// Stockham passes, 8 points per lane, exchange through the wave's own LDS scratch - fft512 of fft_common.h, shared with csrc/mel.hip)
// plus the even/odd split; the inverse runs the same forward FFT on the conjugated, re-merged half spectrum.  The inverse basis
// pinv(scale F)^T window is exactly window * irfft / scale (F has full column rank; the pseudo-inverse projects out the imaginary parts
// of bins 0 and 512, whose basis rows are zero, and inverts the rest), so no dense matrix exists anywhere.
//
// Data layout of a Griffin-Lim run (per utterance b with F_b frames, L_b = hop (F_b - 1) output samples):
//   Y [B][F][1024]  windowed time-domain frames  y_f[n] = w[n] irfft(X_f)[n] / 4        (the conv_transpose1d columns, before overlap-add)
//   s(u) = 4 * (sum_g y_g[u + 512 - 256 g]) / wss(u + 512)                               (overlap-add, window-sum division, n_fft/hop, crop)
// The overlap-add is a GATHER: a sample sums its <= 4 frames in ascending frame order - no atomics, bit-reproducible.  wss is summed in
// the same order from a table of w^2, and the division is skipped where wss <= FLT_MIN (librosa tiny(float32)), like stft.py:111-119.
// One Griffin-Lim iteration (transform of the previous signal, phase kept, magnitude replaced, inverse) is ONE launch from frame buffer
// Y_in to Y_out: each wave gathers the signal under its frame (with the reflect padding of transform at both ends of the utterance, as
// index arithmetic), runs the forward FFT, rescales every bin to the target magnitude (X |X|^-1 = cos / sin of atan2, (1, 0) at |X| = 0),
// runs the inverse FFT and writes its windowed frame.  Ragged batches: per-utterance frame counts; every utterance reflects at its own end.
//
// Fast Griffin-Lim (Perraudin, Balazs, Sondergaard 2013; the momentum of librosa / torchaudio): the same launch with a per-frame STATE
// slot that holds the previous iteration's rebuilt spectrum T.  With X the rebuilt spectrum of this iteration: A = X - coef T, T <- X,
// and A (not X) is rescaled to the target magnitude; coef = momentum / (1 + momentum).  A slot is laid out by lane ownership (what
// split_bins leaves in a lane's registers: float4 (X[k], X[512 - k]) at [m][lane], k = lane + 64 m, then bin 256), is read and rewritten
// by the one wave that owns the frame, each lane its own bytes - in place, no third buffer, no hazard between waves.
// The initial phase can be drawn on the device: theta(b, k, f) = 2 pi u, u in [0, 1) from ctts_mix32 chained over (seed, b, f, k) - a
// pure function of those four, so an utterance's start does not depend on the batch around it, and no [B, 513, F] angle tensor exists.
#include <float.h>
#include "ctts_common.h"
#include "fft_common.h"

namespace {

constexpr int NFFT = 1024, HOP = 256, NBINS = 513;
// workspace layout (floats): the FFT tables [1540] (fft_common.h) | window [1024] | window^2 [1024]
constexpr int WS_WIN = FFT_TW_FLOATS, WS_W2 = WS_WIN + NFFT, WS_FLOATS = WS_W2 + NFFT;
// LDS: the FFT tables and the pass-1 row (fft512_load_tables) | window^2 | 4 waves x scratch
constexpr int LDS_TW1 = FFT_TW_FLOATS, LDS_W2 = FFT_TW_FLOATS + FFT_TW1_FLOATS, LDS_SCR = LDS_W2 + NFFT, LDS_FLOATS = LDS_SCR + 4 * 2 * SCR;
constexpr int MAX_GRID = 1024;             // workgroups of a frame launch: 4 per CU of the 256, each wave walks its frames
constexpr int STATE_SLOT = 4 * 256 + 4;    // floats of a frame's momentum state: float4 (X[k], X[512 - k]) [4][64] | X[256] | 2 floats of padding

// inverse FFT of the spectrum merge_bins left in S, windowed, / (512 * 4) -> one frame of Y (float2 per lane and r: coalesced)
__device__ __forceinline__ void inverse_to_frame(float* S, const float* tw512, const float* tw1, const float (&win)[16], int lane,
                                                 float* __restrict__ yf) {
  float2_ v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) { const int o = pad32(lane + 64 * r); v[r] = {S[2 * o], S[2 * o + 1]}; }
  fft512(v, S, tw512, tw1, lane);
  constexpr float sc = 1.0f / 2048.0f;                  // irfft's 1/512 (of the half-length FFT) and 1/scale = hop / n_fft
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int o = pad32(lane + 64 * r);
    const float re = S[2 * o], im = -S[2 * o + 1];
    reinterpret_cast<float2*>(yf)[lane + 64 * r] = make_float2(win[2 * r] * (re * sc), win[2 * r + 1] * (im * sc));
  }
}

__device__ __forceinline__ void load_tables(float* lds, const float* __restrict__ ws, int tid) {
  fft512_load_tables(lds, ws, tid);
  for (int e = tid; e < NFFT; e += 256) lds[LDS_W2 + e] = ws[WS_W2 + e];
}

// overlap-added, window-sum-normalised, scaled signal at PRE-CROP position t (t = output index + 512) of an utterance with F frames
__device__ __forceinline__ float ola_sample(const float* __restrict__ Yb, const float* w2, int F, int t) {
  const int glo = t >= 768 ? (t - 768) >> 8 : 0, ghi = min(F - 1, t >> 8);
  float acc = 0.f, wss = 0.f;
  for (int g = glo; g <= ghi; ++g) { const int n = t - HOP * g; acc += Yb[(long)g * NFFT + n]; wss += w2[n]; }
  return (wss > FLT_MIN ? acc / wss : acc) * 4.0f;
}
// the same for the pair t, t + 1 (t even: both have the same frames) with 8-byte loads
__device__ __forceinline__ float2_ ola_pair(const float* __restrict__ Yb, const float* w2, int F, int t) {
  const int glo = t >= 768 ? (t - 768) >> 8 : 0, ghi = min(F - 1, t >> 8);
  float a0 = 0.f, a1 = 0.f, s0 = 0.f, s1 = 0.f;
  for (int g = glo; g <= ghi; ++g) {
    const int n = t - HOP * g;
    const float2 y = *reinterpret_cast<const float2*>(Yb + (long)g * NFFT + n);
    a0 += y.x; a1 += y.y; s0 += w2[n]; s1 += w2[n + 1];
  }
  return {(s0 > FLT_MIN ? a0 / s0 : a0) * 4.0f, (s1 > FLT_MIN ? a1 / s1 : a1) * 4.0f};
}

__device__ __forceinline__ void load_window(const float* __restrict__ ws, int lane, float (&win)[16]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) { win[2 * r] = ws[WS_WIN + 2 * (lane + 64 * r)]; win[2 * r + 1] = ws[WS_WIN + 2 * (lane + 64 * r) + 1]; }
}

// ------------------------------------------------------------------------------------------------ STFT.transform: x -> magnitude, phase
__global__ __launch_bounds__(256) void stft_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, const float* __restrict__ ws,
                                                   float* __restrict__ mag, float* __restrict__ phase, long sb, long sk, long sf,
                                                   int B, int N, int F) {
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  load_tables(lds, ws, tid);
  float win[16];
  load_window(ws, lane, win);
  float* S = lds + LDS_SCR + wave * 2 * SCR;
  __syncthreads();
  const long total = (long)B * F;
  for (long gf = (long)blockIdx.x * 4 + wave; gf < total; gf += (long)gridDim.x * 4) {
    const int b = (int)(gf / F), f = (int)(gf - (long)b * F);
    const int Nb = lens ? min(max(lens[b], NFFT / 2 + 1), N) : N;
    const int Fb = 1 + Nb / HOP;
    float* mb = mag + b * sb + f * sf;
    float* pb = phase + b * sb + f * sf;
    if (f >= Fb) {                                      // past this utterance's last frame: zeros
      for (int k = lane; k < NBINS; k += 64) { mb[k * sk] = 0.f; pb[k * sk] = 0.f; }
      continue;
    }
    const float* xb = x + (long)b * N;
    float2_ v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int p = f * HOP + 2 * (lane + 64 * r) - NFFT / 2;
      v[r] = {xb[ctts_reflect_index(p, Nb)] * win[2 * r], xb[ctts_reflect_index(p + 1, Nb)] * win[2 * r + 1]};
    }
    fft512(v, S, lds + WS_W512, lds + LDS_TW1, lane);
    float2_ xk[4], xm[4], x256;
    split_bins(S, lds + WS_W1024, lane, xk, xm, x256);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = lane + 64 * m;
      mb[k * sk] = sqrtf(xk[m].x * xk[m].x + xk[m].y * xk[m].y); pb[k * sk] = atan2f(xk[m].y, xk[m].x);
      mb[(512 - k) * sk] = sqrtf(xm[m].x * xm[m].x + xm[m].y * xm[m].y); pb[(512 - k) * sk] = atan2f(xm[m].y, xm[m].x);
    }
    if (lane == 0) { mb[256 * sk] = sqrtf(x256.x * x256.x + x256.y * x256.y); pb[256 * sk] = atan2f(x256.y, x256.x); }
    CTTS_WAVE_SYNC();
  }
}

// counter-based initial phase: u(seed, b, k, f) in [0, 1) with 24 bits, the dropout kernels' generator chained over b, f and k
constexpr uint32_t GL_PHASE_SITE = 0x474C5048U;          // call-site offset of ctts_drop_key
__device__ __forceinline__ uint32_t phase_frame_key(uint32_t key, int b, int f) {
  return ctts_mix32(ctts_mix32(key + (uint32_t)b * CTTS_DROP_G) + (uint32_t)f * CTTS_DROP_G);
}
__device__ __forceinline__ float phase_u(uint32_t fkey, int k) {
  return (float)(ctts_mix32(fkey + (uint32_t)k * CTTS_DROP_G) >> 8) * (1.0f / 16777216.0f);
}

// ------------------------------------------------------------------------------------------------ inverse, part 1: (mag, phase) -> Y
// SEEDED: the phase is not read but drawn, theta = 2 pi phase_u; (cos, sin)(theta) = sincospi(2 u), exact in the argument
template <bool SEEDED>
__global__ __launch_bounds__(256) void istft_frames_kernel(const float* __restrict__ mag, const float* __restrict__ phase, long sb, long sk, long sf,
                                                           const int32_t* __restrict__ frames, const float* __restrict__ ws,
                                                           float* __restrict__ Y, float* __restrict__ magT, int B, int F,
                                                           const int64_t* __restrict__ seed) {
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  load_tables(lds, ws, tid);
  float win[16];
  load_window(ws, lane, win);
  float* S = lds + LDS_SCR + wave * 2 * SCR;
  uint32_t key = 0;
  if (SEEDED) key = ctts_drop_key(reinterpret_cast<const uint64_t*>(seed), GL_PHASE_SITE);
  __syncthreads();
  const long total = (long)B * F;
  for (long gf = (long)blockIdx.x * 4 + wave; gf < total; gf += (long)gridDim.x * 4) {
    const int b = (int)(gf / F), f = (int)(gf - (long)b * F);
    const int Fb = frames ? min(max(frames[b], 2), F) : F;
    if (f >= Fb) continue;
    const float* mb = mag + b * sb + f * sf;
    const float* pb = SEEDED ? nullptr : phase + b * sb + f * sf;
    const uint32_t fkey = SEEDED ? phase_frame_key(key, b, f) : 0u;
    auto unit = [&](int k, float* s, float* co) {
      if (SEEDED) sincospif(2.0f * phase_u(fkey, k), s, co);
      else sincosf(pb[k * sk], s, co);
    };
    float* mt = magT ? magT + gf * NBINS : nullptr;
    float2_ xk[4], xm[4], x256;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = lane + 64 * m, km = 512 - k;
      const float a = mb[k * sk], c = mb[km * sk];
      float s, co;
      unit(k, &s, &co); xk[m] = {a * co, a * s};
      unit(km, &s, &co); xm[m] = {c * co, c * s};
      if (mt) { mt[k] = a; mt[km] = c; }
    }
    {
      const float a = mb[256 * sk];
      float s, co;
      unit(256, &s, &co);
      x256 = {a * co, a * s};
      if (mt && lane == 0) mt[256] = a;
    }
    merge_bins(S, lds + WS_W1024, lane, xk, xm, x256);
    inverse_to_frame(S, lds + WS_W512, lds + LDS_TW1, win, lane, Y + gf * NFFT);
  }
}

// ------------------------------------------------------------------------------------------------ one Griffin-Lim iteration: Y_in -> Y_out
// MOM: the fast Griffin-Lim update through the frame's state slot (see the head of the file); first: the state counts as zero, is not read
template <bool MOM>
__global__ __launch_bounds__(256) void gl_iter_kernel(const float* __restrict__ Yin, const float* __restrict__ magT, const int32_t* __restrict__ frames,
                                                      const float* __restrict__ ws, float* __restrict__ Yout, int B, int F,
                                                      float* __restrict__ state, float coef, int first) {
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  load_tables(lds, ws, tid);
  float win[16];
  load_window(ws, lane, win);
  float* S = lds + LDS_SCR + wave * 2 * SCR;
  const float* w2 = lds + LDS_W2;
  __syncthreads();
  const long total = (long)B * F;
  for (long gf = (long)blockIdx.x * 4 + wave; gf < total; gf += (long)gridDim.x * 4) {
    const int b = (int)(gf / F), f = (int)(gf - (long)b * F);
    const int Fb = frames ? min(max(frames[b], 4), F) : F;
    if (f >= Fb) continue;
    const int L = HOP * (Fb - 1);
    const float* Yb = Yin + (long)b * F * NFFT;
    // the previous rebuilt spectrum: loaded ahead of the gather and the FFT, which hide its latency
    float4 tp[4] = {};
    float2 tp256 = {};
    float* st = MOM ? state + gf * STATE_SLOT : nullptr;
    if (MOM && !first) {
#pragma unroll
      for (int m = 0; m < 4; ++m) tp[m] = reinterpret_cast<const float4*>(st)[m * 64 + lane];
      if (lane == 0) tp256 = *reinterpret_cast<const float2*>(st + 1024);
    }
    // transform of the previous signal: frame f covers output samples u = 256 f - 512 + n, reflected at 0 and L - 1
    float2_ v[8];
    const int base = f * HOP - NFFT / 2;
    if (base >= 0 && base + NFFT <= L) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float2_ s = ola_pair(Yb, w2, Fb, base + 2 * (lane + 64 * r) + NFFT / 2);
        v[r] = {s.x * win[2 * r], s.y * win[2 * r + 1]};
      }
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int u = base + 2 * (lane + 64 * r);
        v[r] = {ola_sample(Yb, w2, Fb, ctts_reflect_index(u, L) + NFFT / 2) * win[2 * r], ola_sample(Yb, w2, Fb, ctts_reflect_index(u + 1, L) + NFFT / 2) * win[2 * r + 1]};
      }
    }
    fft512(v, S, lds + WS_W512, lds + LDS_TW1, lane);
    float2_ xk[4], xm[4], x256;
    split_bins(S, lds + WS_W1024, lane, xk, xm, x256);
    if (MOM) {                                          // T <- X, then X <- A = X - coef T_prev (bin 256 lives in lane 0 alone: merge_bins)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        reinterpret_cast<float4*>(st)[m * 64 + lane] = make_float4(xk[m].x, xk[m].y, xm[m].x, xm[m].y);
        xk[m] = {xk[m].x - coef * tp[m].x, xk[m].y - coef * tp[m].y};
        xm[m] = {xm[m].x - coef * tp[m].z, xm[m].y - coef * tp[m].w};
      }
      if (lane == 0) *reinterpret_cast<float2*>(st + 1024) = make_float2(x256.x, x256.y);
      x256 = {x256.x - coef * tp256.x, x256.y - coef * tp256.y};
    }
    // keep the phase, take the target magnitude: mag * (cos, sin)(atan2(im, re)) = mag * X / |X|, (mag, 0) where |X| = 0
    const float* mt = magT + gf * NBINS;
    auto rescale = [](float2_ z, float a) -> float2_ {
      const float r = sqrtf(z.x * z.x + z.y * z.y);
      return r > 0.f ? float2_{a * (z.x / r), a * (z.y / r)} : float2_{a, 0.f};
    };
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = lane + 64 * m;
      xk[m] = rescale(xk[m], mt[k]);
      xm[m] = rescale(xm[m], mt[512 - k]);
    }
    x256 = rescale(x256, mt[256]);
    merge_bins(S, lds + WS_W1024, lane, xk, xm, x256);
    inverse_to_frame(S, lds + WS_W512, lds + LDS_TW1, win, lane, Yout + gf * NFFT);
  }
}

// ------------------------------------------------------------------------------------------------ inverse, part 2: Y -> waveform
__global__ __launch_bounds__(256) void istft_ola_kernel(const float* __restrict__ Y, const int32_t* __restrict__ frames, const float* __restrict__ ws,
                                                        float* __restrict__ out, long ld_out, int F) {
  __shared__ float w2[NFFT];
  for (int e = threadIdx.x; e < NFFT; e += 256) w2[e] = ws[WS_W2 + e];
  __syncthreads();
  const int b = blockIdx.y;
  const int Fb = frames ? min(max(frames[b], 2), F) : F;
  const int L = HOP * (Fb - 1), Lmax = HOP * (F - 1);
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= Lmax) return;
  out[(long)b * ld_out + u] = u < L ? ola_sample(Y + (long)b * F * NFFT, w2, Fb, u + NFFT / 2) : 0.f;
}

__global__ void gl_prepare_kernel(const float* __restrict__ window, float* __restrict__ ws) {
  const int tid = threadIdx.x;
  fft512_fill_tables(ws, tid, blockDim.x);
  for (int n = tid; n < NFFT; n += blockDim.x) { const float w = window[n]; ws[WS_WIN + n] = w; ws[WS_W2 + n] = w * w; }
}

int frame_grid(long frames) { const long g = (frames + 3) / 4; return (int)(g < MAX_GRID ? g : MAX_GRID); }

}  // namespace

extern "C" size_t ctts_griffinlim_workspace_bytes(int n_fft, int hop) {
  (void)n_fft; (void)hop;
  return sizeof(float) * (size_t)WS_FLOATS;
}

extern "C" int ctts_griffinlim_prepare(const float* window, int n_fft, int hop, float* workspace, void* stream) {
  CTTS_REQUIRE(window && workspace, "ctts_griffinlim_prepare: null pointer");
  CTTS_REQUIRE(n_fft == NFFT && hop == HOP, "ctts_griffinlim_prepare: built for n_fft = 1024, hop = 256; got %d / %d", n_fft, hop);
  hipLaunchKernelGGL(gl_prepare_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, window, workspace);
  CTTS_CHECK_LAUNCH("ctts_griffinlim_prepare");
  return 0;
}

extern "C" int ctts_stft_transform(const float* x, const int32_t* lens, const float* workspace, float* mag, float* phase, int64_t sb, int64_t sk,
                                   int64_t sf, int B, int N, int n_fft, int hop, void* stream) {
  CTTS_REQUIRE(x && workspace && mag && phase && B > 0, "ctts_stft_transform: bad arguments");
  CTTS_REQUIRE(n_fft == NFFT && hop == HOP, "ctts_stft_transform: built for n_fft = 1024, hop = 256; got %d / %d", n_fft, hop);
  CTTS_REQUIRE(N > NFFT / 2, "ctts_stft_transform: reflect padding needs more than n_fft/2 samples (got %d)", N);
  const int F = 1 + N / HOP;
  hipLaunchKernelGGL(stft_kernel, dim3(frame_grid((long)B * F)), dim3(256), 0, (hipStream_t)stream, x, lens, workspace, mag, phase,
                     (long)sb, (long)sk, (long)sf, B, N, F);
  CTTS_CHECK_LAUNCH("ctts_stft_transform");
  return 0;
}

extern "C" int ctts_istft_frames(const float* mag, const float* phase, int64_t sb, int64_t sk, int64_t sf, const int32_t* frames,
                                 const float* workspace, float* Y, float* magT, int B, int F, int n_fft, int hop, void* stream) {
  CTTS_REQUIRE(mag && phase && workspace && Y && B > 0, "ctts_istft_frames: bad arguments");
  CTTS_REQUIRE(n_fft == NFFT && hop == HOP, "ctts_istft_frames: built for n_fft = 1024, hop = 256; got %d / %d", n_fft, hop);
  CTTS_REQUIRE(F >= 2, "ctts_istft_frames: needs at least 2 frames (got %d)", F);
  hipLaunchKernelGGL(istft_frames_kernel<false>, dim3(frame_grid((long)B * F)), dim3(256), 0, (hipStream_t)stream, mag, phase, (long)sb,
                     (long)sk, (long)sf, frames, workspace, Y, magT, B, F, (const int64_t*)nullptr);
  CTTS_CHECK_LAUNCH("ctts_istft_frames");
  return 0;
}

extern "C" int ctts_istft_frames_seeded(const float* mag, int64_t sb, int64_t sk, int64_t sf, const int32_t* frames, const float* workspace,
                                        const int64_t* seed, float* Y, float* magT, int B, int F, int n_fft, int hop, void* stream) {
  CTTS_REQUIRE(mag && workspace && seed && Y && B > 0, "ctts_istft_frames_seeded: bad arguments");
  CTTS_REQUIRE(n_fft == NFFT && hop == HOP, "ctts_istft_frames_seeded: built for n_fft = 1024, hop = 256; got %d / %d", n_fft, hop);
  CTTS_REQUIRE(F >= 2, "ctts_istft_frames_seeded: needs at least 2 frames (got %d)", F);
  hipLaunchKernelGGL(istft_frames_kernel<true>, dim3(frame_grid((long)B * F)), dim3(256), 0, (hipStream_t)stream, mag, (const float*)nullptr,
                     (long)sb, (long)sk, (long)sf, frames, workspace, Y, magT, B, F, seed);
  CTTS_CHECK_LAUNCH("ctts_istft_frames_seeded");
  return 0;
}

extern "C" int ctts_griffinlim_iter(const float* Y_in, const float* magT, const int32_t* frames, const float* workspace, float* Y_out, int B,
                                    int F, int n_fft, int hop, void* stream) {
  CTTS_REQUIRE(Y_in && magT && workspace && Y_out && Y_in != Y_out && B > 0, "ctts_griffinlim_iter: bad arguments");
  CTTS_REQUIRE(n_fft == NFFT && hop == HOP, "ctts_griffinlim_iter: built for n_fft = 1024, hop = 256; got %d / %d", n_fft, hop);
  CTTS_REQUIRE(F >= 4, "ctts_griffinlim_iter: needs at least 4 frames (got %d)", F);
  hipLaunchKernelGGL(gl_iter_kernel<false>, dim3(frame_grid((long)B * F)), dim3(256), 0, (hipStream_t)stream, Y_in, magT, frames, workspace,
                     Y_out, B, F, (float*)nullptr, 0.f, 0);
  CTTS_CHECK_LAUNCH("ctts_griffinlim_iter");
  return 0;
}

extern "C" size_t ctts_griffinlim_state_floats(int B, int F) {
  return B > 0 && F > 0 ? (size_t)B * (size_t)F * STATE_SLOT : 0;
}

extern "C" int ctts_griffinlim_iter_momentum(const float* Y_in, const float* magT, float* state, const int32_t* frames, const float* workspace,
                                             float* Y_out, float coef, int first, int B, int F, int n_fft, int hop, void* stream) {
  CTTS_REQUIRE(Y_in && magT && state && workspace && Y_out && Y_in != Y_out && B > 0, "ctts_griffinlim_iter_momentum: bad arguments");
  CTTS_REQUIRE(n_fft == NFFT && hop == HOP, "ctts_griffinlim_iter_momentum: built for n_fft = 1024, hop = 256; got %d / %d", n_fft, hop);
  CTTS_REQUIRE(F >= 4, "ctts_griffinlim_iter_momentum: needs at least 4 frames (got %d)", F);
  CTTS_REQUIRE(coef >= 0.f && coef < 1.f, "ctts_griffinlim_iter_momentum: coef = momentum / (1 + momentum) must lie in [0, 1), got %g", (double)coef);
  hipLaunchKernelGGL(gl_iter_kernel<true>, dim3(frame_grid((long)B * F)), dim3(256), 0, (hipStream_t)stream, Y_in, magT, frames, workspace,
                     Y_out, B, F, state, coef, first);
  CTTS_CHECK_LAUNCH("ctts_griffinlim_iter_momentum");
  return 0;
}

extern "C" int ctts_istft_ola(const float* Y, const int32_t* frames, const float* workspace, float* out, int64_t ld_out, int B, int F, int n_fft,
                              int hop, void* stream) {
  CTTS_REQUIRE(Y && workspace && out && B > 0, "ctts_istft_ola: bad arguments");
  CTTS_REQUIRE(n_fft == NFFT && hop == HOP, "ctts_istft_ola: built for n_fft = 1024, hop = 256; got %d / %d", n_fft, hop);
  CTTS_REQUIRE(F >= 2 && ld_out >= (int64_t)HOP * (F - 1), "ctts_istft_ola: needs F >= 2 frames and ld_out >= hop (F - 1)");
  const int L = HOP * (F - 1);
  hipLaunchKernelGGL(istft_ola_kernel, dim3((L + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, Y, frames, workspace, out, (long)ld_out, F);
  CTTS_CHECK_LAUNCH("ctts_istft_ola");
  return 0;
}
