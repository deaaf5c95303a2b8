// Audio resampling on the device (include/ctts.h "Audio resampling on the device"): the band-limited rate change
// every entry into the reference's data path performs on the host (librosa.load(path, sr): preprocessor.py:364, :460, vctk.py:31) and the
// peak normalisation + int16 cast that follow it in prepare_align (vctk.py:32-36).
//
// resample_kernel - exact-phase polyphase FIR, y[n] = sum_j bank[r][j] x[k - j] with t = n M + half, r = t mod L, k = t div L.  Outputs
//   n and n + L share the coefficient row r and read inputs M apart, so the work is laid out by PERIODS: a tile is P consecutive periods
//   (P L consecutive outputs), one wave takes one phase c (one row r) and its 64 lanes take 64 consecutive periods.  The coefficient is
//   then wave-uniform: it arrives through the scalar cache (eight per chunk; the compiler pairs two chunks into one s_load_dwordx16)
//   as the SGPR operand of v_fmac_f32 and costs no vector-memory or LDS traffic; the only per-FMA
//   operand fetch is one ds_read_b32 of the input, which the whole workgroup staged once (zero-filled outside [0, len)).
//   LDS image: one row per period, row rho holds input positions [base + rho M - 7, base + rho M + M), i.e. M samples behind 7 samples of
//   halo copied from the row before, at a row stride of (M + 7) | 1 words.  The halo lets a chunk of eight taps be read at immediate
//   offsets from one address whatever its phase; the odd stride puts the 64 lanes of a read (consecutive rows, same column) on distinct
//   banks - at M = 320 the unpadded stride of 320 words would land all 32 lanes of a group on one bank.
//   Every output is one thread's fmaf chain over j = 0 .. T-1 in that order: no atomics, no dependence on B, on other rows or on the grid.
// copy_kernel - L == M.  peak_*_kernel - max |x| per utterance (integer max on the bits of |x|: exact in any order), then the quantiser.
#include "ctts_common.h"
#include <math.h>

namespace {

constexpr int RS_THREADS = 1024, RS_WAVES = RS_THREADS / 64;
constexpr int RS_CHUNK = 8, RS_HALO = RS_CHUNK - 1;    // taps per coefficient load; halo samples in front of every LDS row
constexpr int RS_LDS_FLOATS = 39936;                   // 156 KiB of the CU's 160: one workgroup of 16 waves per CU
constexpr int RS_STAGE = 8;                             // global loads a thread keeps in flight while it stages the tile's input
constexpr int RS_TARGET_ITEMS = 128;                   // (phase, period block) pairs a tile should offer its 16 waves
constexpr int RS_MAX_LM = 1024, RS_MAX_T = 1024, RS_MAX_SPLIT = 8;
constexpr long RS_MAX_N = 1L << 30;
constexpr int PK_THREADS = 256, PK_CHUNK = 4096;       // samples per workgroup of the peak / quantise kernels

struct rs_plan {
  int lanes;     // periods per wave (64, fewer only when 64 rows of M + 7 samples do not fit the LDS)
  int W;         // period blocks per tile
  int rows;      // LDS rows
  int mrow;      // LDS row stride in words
  int drows;     // rows in front of the tile's first period (taps reach back T - 1 samples)
  int rw_log;    // staging: log2 of the lanes that share one row
  int dq, dr;    // RS_CHUNK = dq M + dr
};

bool rs_make_plan(int L, int M, int T, int half, rs_plan* p) {
  if (L < 1 || M < 1 || L > RS_MAX_LM || M > RS_MAX_LM || T < RS_CHUNK || T > RS_MAX_T || T % RS_CHUNK || half < 0 ||
      2L * half + 1 > (long)L * T)
    return false;
  p->mrow = (M + RS_HALO) | 1;
  const int kc0 = half / L, kc1 = (int)(((long)(L - 1) * M + half) / L);       // k - p M of the first / last phase
  p->drows = T - 1 > kc0 ? (T - 1 - kc0 + M - 1) / M : 0;
  const int extra = (kc1 + p->drows * M) / M + 1;
  p->lanes = 64;
  while (p->lanes > 1 && (long)(p->lanes + extra) * p->mrow > RS_LDS_FLOATS) p->lanes >>= 1;
  if ((long)(p->lanes + extra) * p->mrow > RS_LDS_FLOATS) return false;
  p->W = 1;
  if (p->lanes == 64) {
    const int fit = (RS_LDS_FLOATS / p->mrow - extra) / 64, want = (RS_TARGET_ITEMS + L - 1) / L;
    p->W = want < fit ? want : fit;
    if (p->W < 1) p->W = 1;
  }
  p->rows = p->lanes * p->W + extra;
  p->rw_log = 3;
  while (p->rw_log < 6 && (1 << p->rw_log) < M + RS_HALO) ++p->rw_log;
  p->dq = RS_CHUNK / M;
  p->dr = RS_CHUNK % M;
  return true;
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens,
                                                              const float* __restrict__ bank, float* __restrict__ out,
                                                              int32_t* __restrict__ out_lens, int N, int No, int L, int M, int T, int half,
                                                              rs_plan pl, int S) {
  extern __shared__ float xs[];
  const int b = blockIdx.y, tile = blockIdx.x / S, cs = blockIdx.x - tile * S;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int len = min(max(lens[b], 0), N);
  const int olen = (int)(((long)len * L + M - 1) / M);
  if (blockIdx.x == 0 && threadIdx.x == 0) out_lens[b] = olen;
  const int P = pl.lanes * pl.W;
  const long p0 = (long)tile * P;                                  // first period of the tile; its outputs start at p0 L
  const bool live = p0 * L < olen;                                 // workgroup-uniform
  if (live) {
    const float* x = wav + (long)b * N;
    const long base = (p0 - pl.drows) * M - RS_HALO;               // input position of LDS row 0, column 0
    const int rw = 1 << pl.rw_log, per = 64 >> pl.rw_log, width = M + RS_HALO;
    for (int rho = wave * per + (lane >> pl.rw_log); rho < pl.rows; rho += RS_WAVES * per) {
      const long rb = base + (long)rho * M;
      for (int u0 = lane & (rw - 1); u0 < width; u0 += RS_STAGE * rw) {
        // RS_STAGE loads in flight per thread (one at a time, a workgroup spends its first microseconds on round trips).  The index is
        // clamped into the utterance, so nothing at or beyond len is touched; what lies outside [0, len) is then replaced by 0.
        float v[RS_STAGE];
#pragma unroll
        for (int q = 0; q < RS_STAGE; ++q) v[q] = x[min(max(rb + u0 + q * rw, 0L), (long)len - 1)];
#pragma unroll
        for (int q = 0; q < RS_STAGE; ++q) asm volatile("" : "+v"(v[q]));      // keeps all the loads ahead of the range tests
#pragma unroll
        for (int q = 0; q < RS_STAGE; ++q) {
          const long pos = rb + u0 + q * rw;
          v[q] = (pos >= 0 && pos < len) ? v[q] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < RS_STAGE; ++q)
          if (u0 + q * rw < width) xs[rho * pl.mrow + u0 + q * rw] = v[q];
      }
    }
  }
  __syncthreads();
  const int total = L * pl.W, ipc = (total + S - 1) / S;
  const int it1 = min(total, (cs + 1) * ipc);
  float* o = out + (long)b * No;
  for (int it = cs * ipc + wave; it < it1; it += RS_WAVES) {       // wave-uniform
    const int w = it / L, c = it - w * L;
    const int t = c * M + half, kc = t / L, r = t - kc * L;
    const int pi = w * pl.lanes + min(lane, pl.lanes - 1);         // idle lanes (lanes < 64) read a valid row and store nothing
    float acc = 0.f;
    if (live) {
      const int e = kc + pl.drows * M;                             // tap j of period p reads LDS position (p - p0) M + e - j, past the halo
      int rowq = e / M, off = e - rowq * M;
      const float* xl = xs + pi * pl.mrow + RS_HALO;
      const float* brow = bank + (long)r * T;
      for (int j = 0; j < T; j += RS_CHUNK) {
        const float4 c0 = *reinterpret_cast<const float4*>(brow + j), c1 = *reinterpret_cast<const float4*>(brow + j + 4);
        const float* xp = xl + rowq * pl.mrow + off;
        acc = fmaf(c0.x, xp[0], acc);
        acc = fmaf(c0.y, xp[-1], acc);
        acc = fmaf(c0.z, xp[-2], acc);
        acc = fmaf(c0.w, xp[-3], acc);
        acc = fmaf(c1.x, xp[-4], acc);
        acc = fmaf(c1.y, xp[-5], acc);
        acc = fmaf(c1.z, xp[-6], acc);
        acc = fmaf(c1.w, xp[-7], acc);
        off -= pl.dr;
        rowq -= pl.dq;
        if (off < 0) { off += M; --rowq; }
      }
    }
    const long n = (p0 + pi) * L + c;
    if (lane < pl.lanes && n < No) o[n] = n < olen ? acc : 0.f;
  }
}

__global__ __launch_bounds__(256) void copy_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, float* __restrict__ out,
                                                   int32_t* __restrict__ out_lens, int N) {
  const int b = blockIdx.y;
  const int len = min(max(lens[b], 0), N);
  if (blockIdx.x == 0 && threadIdx.x == 0) out_lens[b] = len;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < N) out[(long)b * N + i] = i < len ? wav[(long)b * N + i] : 0.f;
}

// peak_bits[b] = bits of max |x[i]|, i < len: non-negative floats order like their bit patterns, and an integer maximum is exact in any order
__global__ __launch_bounds__(PK_THREADS) void peak_max_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens,
                                                              unsigned* __restrict__ peak_bits, int N) {
  __shared__ float red[PK_THREADS / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const long i0 = (long)blockIdx.x * PK_CHUNK;
  if (i0 >= len) return;                                           // workgroup-uniform
  const float* x = wav + (long)b * N;
  const long i1 = min(i0 + PK_CHUNK, (long)len);
  float m = 0.f;
  for (long i = i0 + tid; i < i1; i += PK_THREADS) m = fmaxf(m, fabsf(x[i]));
  m = ctts_wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(peak_bits + b, __float_as_uint(m));
  }
}

__global__ __launch_bounds__(PK_THREADS) void peak_quantise_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens,
                                                                   const float* __restrict__ peak, float* __restrict__ out,
                                                                   int16_t* __restrict__ q16, int32_t* __restrict__ valid, int N,
                                                                   float max_wav_value) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const float pk = peak[b];
  if (blockIdx.x == 0 && tid == 0) valid[b] = pk > 0.f ? 1 : 0;
  const long i0 = (long)blockIdx.x * PK_CHUNK, i1 = min(i0 + PK_CHUNK, (long)N);
  const float* x = wav + (long)b * N;
  for (long i = i0 + tid; i < i1; i += PK_THREADS) {
    float q = 0.f;
    if (i < len && pk > 0.f) {
      const float v = __fmul_rn(__fdiv_rn(x[i], pk), max_wav_value);   // numpy on a float32 array: an IEEE division, then one multiply
      q = fminf(fmaxf(truncf(v), -32768.f), 32767.f);
    }
    out[(long)b * N + i] = q * (1.0f / 32768.0f);
    if (q16) q16[(long)b * N + i] = (int16_t)q;
  }
}

}  // namespace

extern "C" int ctts_resample_tile(int L, int M, int T, int half) {
  rs_plan p;
  if (L == M || !rs_make_plan(L, M, T, half, &p)) return 0;
  return p.lanes * p.W * L;
}

extern "C" int ctts_resample(const float* wav, const int32_t* lens, const float* bank, float* out, int32_t* out_lens, int B, int N, int L, int M,
                             int T, int half, void* stream) {
  CTTS_REQUIRE(wav && lens && out && out_lens && B > 0 && N > 0, "ctts_resample: bad arguments");
  CTTS_REQUIRE(B <= 65535, "ctts_resample: at most 65535 utterances per call (got %d)", B);
  CTTS_REQUIRE(L >= 1 && M >= 1 && L <= RS_MAX_LM && M <= RS_MAX_LM, "ctts_resample: need 1 <= L, M <= %d (got %d / %d)", RS_MAX_LM, L, M);
  const long No = ((long)N * L + M - 1) / M;
  CTTS_REQUIRE(N <= RS_MAX_N && No <= RS_MAX_N, "ctts_resample: at most 2^30 samples per row on either side (got %d -> %ld)", N, No);
  hipStream_t st = (hipStream_t)stream;
  if (L == M) {
    hipLaunchKernelGGL(copy_kernel, dim3((N + 255) / 256, B), dim3(256), 0, st, wav, lens, out, out_lens, N);
    CTTS_CHECK_LAUNCH("ctts_resample (copy)");
    return 0;
  }
  CTTS_REQUIRE(bank && ((uintptr_t)bank & 31) == 0, "ctts_resample: the coefficient bank must be given, 32-byte aligned");
  CTTS_REQUIRE(T >= RS_CHUNK && T <= RS_MAX_T && T % RS_CHUNK == 0, "ctts_resample: need T a multiple of %d in [%d, %d] (got %d)", RS_CHUNK, RS_CHUNK,
               RS_MAX_T, T);
  CTTS_REQUIRE(half >= 0 && 2L * half + 1 <= (long)L * T, "ctts_resample: the bank [%d][%d] does not hold 2 * %d + 1 taps", L, T, half);
  rs_plan p;
  CTTS_REQUIRE(rs_make_plan(L, M, T, half, &p), "ctts_resample: no tile of %d -> %d with %d taps per phase fits the LDS", M, L, T);
  const long tile_out = (long)p.lanes * p.W * L, tiles = (No + tile_out - 1) / tile_out;
  // phases of a tile are split over S workgroups when the tiles alone would leave compute units idle (each stages the tile's input again)
  int S = 1;
  while (S < RS_MAX_SPLIT && tiles * B * S < 512 && (L * p.W) / (2 * S) >= RS_WAVES) S *= 2;
  CTTS_REQUIRE(tiles * S <= 0x7fffffffL, "ctts_resample: too many tiles");
  const size_t lds_bytes = sizeof(float) * (size_t)p.rows * p.mrow;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * RS_LDS_FLOATS));
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(tiles * S), B), dim3(RS_THREADS), lds_bytes, st, wav, lens, bank, out, out_lens, N, (int)No, L,
                     M, T, half, p, S);
  CTTS_CHECK_LAUNCH("ctts_resample");
  return 0;
}

extern "C" int ctts_peak_normalize(const float* wav, const int32_t* lens, float* out, int16_t* out_i16, float* peak, int32_t* valid, int B, int N,
                                   float max_wav_value, void* stream) {
  CTTS_REQUIRE(wav && lens && out && peak && valid && B > 0 && N > 0, "ctts_peak_normalize: bad arguments");
  CTTS_REQUIRE(B <= 65535, "ctts_peak_normalize: at most 65535 utterances per call (got %d)", B);
  CTTS_REQUIRE(max_wav_value > 0.f && max_wav_value < INFINITY, "ctts_peak_normalize: max_wav_value must be positive and finite (got %g)",
               (double)max_wav_value);
  hipStream_t st = (hipStream_t)stream;
  if (ctts_zero_async(peak, sizeof(float) * (size_t)B, st) != 0) return -2;
  const dim3 grid((N + PK_CHUNK - 1) / PK_CHUNK, B);
  hipLaunchKernelGGL(peak_max_kernel, grid, dim3(PK_THREADS), 0, st, wav, lens, reinterpret_cast<unsigned*>(peak), N);
  CTTS_CHECK_LAUNCH("ctts_peak_normalize (peak)");
  hipLaunchKernelGGL(peak_quantise_kernel, grid, dim3(PK_THREADS), 0, st, wav, lens, peak, out, out_i16, valid, N, max_wav_value);
  CTTS_CHECK_LAUNCH("ctts_peak_normalize");
  return 0;
}
