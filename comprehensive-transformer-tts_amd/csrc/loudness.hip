// Loudness metering and normalisation on the device (include/ctts.h "Loudness on the device"): ITU-R BS.1770
// integrated loudness as the reference takes it on the host with pyloudnorm before feature extraction (audio/stft.py:226-231).
//
// K-weighting is two biquads in cascade, a 4th-order recursion whose high-pass poles sit at about 1 - 2 pi 38 / rate: a sample depends
// on thousands of predecessors.  Each utterance is cut into CHUNKS of LD_CHUNK samples anchored at its own sample 0 and the four-word
// filter state is chained across them by launch order, never by one workgroup waiting on another:
//   kweight_kernel<false>  every full chunk that has a successor is filtered from the ZERO state by one lane; its final state f_c
//                          (transposed direct form II words of both sections, double) goes to the workspace.
//   scan_kernel            one workgroup per utterance turns f_c into the true state at the end of every chunk, s_c = P s_{c-1} + f_c
//                          with P = A^LD_CHUNK (A: the cascade's 4 x 4 state transition): a scan in groups of 16 over as many levels as
//                          the utterance needs, with the host-made powers P^(16^l m), m = 1 .. 16.  Groups are counted from chunk 0, so
//                          the order of every sum depends on the chunk index alone.
//   kweight_kernel<true>   filters every chunk again from its true state and adds y^2 to the hop segment the sample falls in.  A tile
//                          (one wave, 64 chunks) holds one partial per lane and segment in LDS and sums them in lane order; the result
//                          is hop_sums[b][tile][slot].  Also max |x| per utterance (integer max on the bits: exact in any order).
//   gate_kernel            one workgroup per utterance: segments from tile partials, blocks from segments, the two gates, the gain.
// The filtered signal is never stored.  All recursion state, products and sums are double; the samples are fp32 and enter exactly.
// Block edges come from the host as integers (the definition evaluates them in floating point: int(0.4 (j 0.25) rate)), so the device
// and the float64 restatement cut at the same samples.  Nothing depends on B, on N, on other rows or on the grid.
#include "ctts_common.h"
#include <math.h>
#include <limits.h>

namespace {

constexpr int LD_CHUNK = 128;                    // samples one lane filters
constexpr int LD_TILE = 64 * LD_CHUNK;           // samples one wave (= one workgroup) stages
constexpr int LD_STAGE = 32;                     // global loads a lane keeps in flight while it stages the tile
constexpr int LD_ROW = LD_CHUNK + 1;             // LDS row stride in words: odd, the 64 lanes of a read fall on distinct banks
constexpr int LD_SLOTS = 16;                     // hop segments a tile may touch (the host refuses tables that need more)
constexpr int LD_FAN = 16, LD_LEVELS = 5;        // scan: group size, levels (16^5 chunks and more than ctts allows per row)
constexpr int LD_COEF_DOUBLES = 16 + LD_LEVELS * LD_FAN * 16;
constexpr int LD_MAX_N = 1 << 24;
constexpr int LD_MAX_SEGS = 3072;                // hop segments / blocks per utterance the gate holds in LDS
constexpr int LD_GATE_THREADS = 256;
constexpr int AG_THREADS = 256;

struct ld_levels {
  int off[LD_LEVELS];      // first slot of level l inside an utterance's workspace (slots of 4 doubles)
  int stride;              // slots per utterance
};

ld_levels ld_make_levels(int N) {
  ld_levels lv;
  int cnt = (N + LD_CHUNK - 1) / LD_CHUNK, off = 0;
  for (int l = 0; l < LD_LEVELS; ++l) {
    lv.off[l] = off;
    off += cnt;
    cnt /= LD_FAN;
  }
  lv.stride = off;
  return lv;
}

struct ld_state {
  double a1, a2, b1, b2;   // z1, z2 of the shelf; z1, z2 of the high pass
};

__device__ __forceinline__ ld_state ld_mul_add(const double* __restrict__ m, const ld_state& s, const ld_state& f) {
  ld_state r;
  r.a1 = fma(m[0], s.a1, fma(m[1], s.a2, fma(m[2], s.b1, fma(m[3], s.b2, f.a1))));
  r.a2 = fma(m[4], s.a1, fma(m[5], s.a2, fma(m[6], s.b1, fma(m[7], s.b2, f.a2))));
  r.b1 = fma(m[8], s.a1, fma(m[9], s.a2, fma(m[10], s.b1, fma(m[11], s.b2, f.b1))));
  r.b2 = fma(m[12], s.a1, fma(m[13], s.a2, fma(m[14], s.b1, fma(m[15], s.b2, f.b2))));
  return r;
}

__device__ __forceinline__ ld_state ld_load(const double* p) { return {p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void ld_store(double* p, const ld_state& s) {
  p[0] = s.a1;
  p[1] = s.a2;
  p[2] = s.b1;
  p[3] = s.b2;
}

template <bool ENERGY>
__global__ __launch_bounds__(64) void kweight_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens,
                                                     const double* __restrict__ coef, const int32_t* __restrict__ edges,
                                                     const int32_t* __restrict__ chunk_seg, double* __restrict__ ws,
                                                     double* __restrict__ hop_sums, unsigned* __restrict__ peak_bits, int N, int n_edges,
                                                     int ntiles, int ws_stride) {
  __shared__ float xs[64 * LD_ROW];
  __shared__ double part[ENERGY ? 64 * LD_SLOTS : 1];
  const int b = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const int t0 = tile * LD_TILE;
  if (t0 >= len) return;                                            // workgroup-uniform
  const int nch = (len + LD_CHUNK - 1) / LD_CHUNK;                  // chunks of this utterance; the last one may be short
  if (!ENERGY && tile * 64 + 1 >= nch) return;                      // no chunk of this tile has a successor
  const float* x = wav + (long)b * N;
  // one wave per SIMD is all the parallelism a batch of utterances offers, so the loads' latency is hidden by keeping LD_STAGE of
  // them in flight per lane, not by other waves
  for (int i0 = 0; i0 < LD_TILE; i0 += 64 * LD_STAGE) {
    float v[LD_STAGE];
#pragma unroll
    for (int q = 0; q < LD_STAGE; ++q) v[q] = x[min(t0 + i0 + q * 64 + lane, len - 1)];      // clamped: nothing at or beyond len is read
#pragma unroll
    for (int q = 0; q < LD_STAGE; ++q) asm volatile("" : "+v"(v[q]));                        // keeps all the loads ahead of the range tests
#pragma unroll
    for (int q = 0; q < LD_STAGE; ++q) {
      const int idx = i0 + q * 64 + lane;
      xs[(idx / LD_CHUNK) * LD_ROW + (idx % LD_CHUNK)] = t0 + idx < len ? v[q] : 0.f;
    }
  }
  if (ENERGY)
    for (int i = lane; i < 64 * LD_SLOTS; i += 64) part[i] = 0.0;
  __syncthreads();
  const double sb0 = coef[0], sb1 = coef[1], sb2 = coef[2], sa1 = coef[3], sa2 = coef[4];
  const double hb0 = coef[5], hb1 = coef[6], hb2 = coef[7], ha1 = coef[8], ha2 = coef[9];
  const int c = tile * 64 + lane, start = t0 + lane * LD_CHUNK;
  const int nv = min(max(len - start, 0), LD_CHUNK);
  double* wsb = ws + (long)b * ws_stride * 4;
  ld_state s = {0.0, 0.0, 0.0, 0.0};
  int slot = 0, k = 0, next = INT_MAX;
  if (ENERGY) {
    if (c > 0 && nv > 0) s = ld_load(wsb + (long)(c - 1) * 4);
    k = chunk_seg[min(c, nch - 1)];
    slot = k - chunk_seg[tile * 64];
    next = (k + 1 < n_edges ? edges[k + 1] : INT_MAX) - start;      // samples of this chunk before the next edge
  }
  const float* xr = xs + lane * LD_ROW;
  double acc = 0.0;
  float pk = 0.f;
#pragma unroll 4
  for (int i = 0; i < LD_CHUNK; ++i) {
    const float xf = xr[i];
    const double xd = (double)xf;
    const double u = fma(sb0, xd, s.a1);
    s.a1 = fma(-sa1, u, fma(sb1, xd, s.a2));
    s.a2 = fma(-sa2, u, sb2 * xd);
    const double y = fma(hb0, u, s.b1);
    s.b1 = fma(-ha1, y, fma(hb1, u, s.b2));
    s.b2 = fma(-ha2, y, hb2 * u);
    if (ENERGY) {
      if (i == next) {                                              // sample i is the first of the next segment
        if (slot >= 0 && slot < LD_SLOTS) part[lane * LD_SLOTS + slot] = acc;
        acc = 0.0;
        ++slot;
        ++k;
        next = (k + 1 < n_edges ? edges[k + 1] : INT_MAX) - start;
      }
      acc = i < nv ? fma(y, y, acc) : acc;
      pk = fmaxf(pk, fabsf(xf));
    }
  }
  if (!ENERGY) {
    if (c + 1 < nch) ld_store(wsb + (long)c * 4, s);
    return;
  }
  if (slot >= 0 && slot < LD_SLOTS) part[lane * LD_SLOTS + slot] = acc;
  pk = ctts_wave_max(pk);
  if (lane == 0) atomicMax(peak_bits + b, __float_as_uint(pk));
  __syncthreads();
  if (lane < LD_SLOTS) {
    double t = 0.0;
    for (int l = 0; l < 64; ++l) t += part[l * LD_SLOTS + lane];    // lane order: the same sum whatever the batch
    hop_sums[((long)b * ntiles + tile) * LD_SLOTS + lane] = t;
  }
}

// s_c = P s_{c-1} + f_c over the n0 = nch - 1 chunk states of one utterance, in place (kernel comment at the top of the file)
__global__ __launch_bounds__(256) void scan_kernel(const int32_t* __restrict__ lens, const double* __restrict__ coef, double* __restrict__ ws,
                                                   int N, ld_levels lv) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const int n0 = (len + LD_CHUNK - 1) / LD_CHUNK - 1;
  if (n0 <= 1) return;
  double* base = ws + (long)b * lv.stride * 4;
  const double* pw = coef + 16;
  int n[LD_LEVELS + 1];                                             // items per level: a level above exists while a level has more than one group
  n[0] = n0;
#pragma unroll
  for (int l = 1; l <= LD_LEVELS; ++l) n[l] = (l < LD_LEVELS && n[l - 1] > LD_FAN) ? n[l - 1] / LD_FAN : 0;
#pragma unroll
  for (int l = 0; l < LD_LEVELS; ++l) {
    if (n[l] > 0) {                                                 // workgroup-uniform
      double* v = base + (long)lv.off[l] * 4;
      double* up = base + (long)lv.off[l + 1 < LD_LEVELS ? l + 1 : l] * 4;      // written only while g < nup
      const int nup = n[l + 1];
      const double* m = pw + (long)(l * LD_FAN) * 16;
      for (int g = tid; g * LD_FAN < n[l]; g += 256) {
        const int cnt = min(n[l] - g * LD_FAN, LD_FAN);
        double* vg = v + (long)g * LD_FAN * 4;
        ld_state f[LD_FAN];
#pragma unroll
        for (int i = 0; i < LD_FAN; ++i) f[i] = i < cnt ? ld_load(vg + i * 4) : ld_state{0.0, 0.0, 0.0, 0.0};      // all loads ahead of the chain
        ld_state s = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < LD_FAN; ++i) {
          if (i < cnt) {
            s = ld_mul_add(m, s, f[i]);
            ld_store(vg + i * 4, s);
          }
        }
        if (g < nup) ld_store(up + (long)g * 4, s);
      }
    }
    __threadfence_block();
    __syncthreads();
  }
#pragma unroll
  for (int l = LD_LEVELS - 2; l >= 0; --l) {
    if (n[l + 1] > 0) {
      double* v = base + (long)lv.off[l] * 4;
      const double* up = base + (long)lv.off[l + 1] * 4;
      for (int i = LD_FAN + tid; i < n[l]; i += 256) {
        const ld_state carry = ld_load(up + (long)(i / LD_FAN - 1) * 4);
        const ld_state s = ld_mul_add(pw + (long)(l * LD_FAN + i % LD_FAN) * 16, carry, ld_load(v + (long)i * 4));
        ld_store(v + (long)i * 4, s);
      }
    }
    __threadfence_block();
    __syncthreads();
  }
}

__global__ __launch_bounds__(LD_GATE_THREADS) void gate_kernel(const double* __restrict__ hop_sums, const int32_t* __restrict__ lens,
                                                               const int32_t* __restrict__ n_blocks, const int32_t* __restrict__ edges,
                                                               const int32_t* __restrict__ chunk_seg, const int32_t* __restrict__ blocks,
                                                               const float* __restrict__ peak, double* __restrict__ loudness,
                                                               float* __restrict__ gain, int32_t* __restrict__ valid,
                                                               double* __restrict__ curve, int N, int n_edges, int J, int ntiles,
                                                               double inv_block, double target, int peak_limit) {
  __shared__ double seg[LD_MAX_SEGS];
  __shared__ double z[LD_MAX_SEGS];
  __shared__ double red[LD_GATE_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const int nb = min(min(max(n_blocks[b], 0), J), LD_MAX_SEGS);
  const int nseg = nb > 0 ? min(min(blocks[2 * (nb - 1) + 1], n_edges - 1), LD_MAX_SEGS) : 0;
  const double* hs = hop_sums + (long)b * ntiles * LD_SLOTS;
  for (int k = tid; k < nseg; k += LD_GATE_THREADS) {
    const int e0 = edges[k], e1 = min(edges[k + 1], len);
    double t = 0.0;
    if (e0 < e1)
      for (int tl = e0 / LD_TILE; tl <= (e1 - 1) / LD_TILE; ++tl) {
        const int slot = k - chunk_seg[tl * 64];
        if (slot >= 0 && slot < LD_SLOTS) t += hs[(long)tl * LD_SLOTS + slot];
      }
    seg[k] = t;
  }
  __syncthreads();
  for (int j = tid; j < nb; j += LD_GATE_THREADS) {
    const int k0 = max(blocks[2 * j], 0), k1 = min(blocks[2 * j + 1], nseg);
    double t = 0.0;
    for (int k = k0; k < k1; ++k) t += seg[k];
    z[j] = t * inv_block;                                           // the divisor is the whole block even where the block was cut at len
  }
  __syncthreads();
  if (curve)
    for (int j = tid; j < J; j += LD_GATE_THREADS) curve[(long)b * J + j] = j < nb ? -0.691 + 10.0 * log10(z[j]) : -INFINITY;
  double s = 0.0, cnt = 0.0;
  for (int j = tid; j < nb; j += LD_GATE_THREADS)
    if (-0.691 + 10.0 * log10(z[j]) >= -70.0) {
      s += z[j];
      cnt += 1.0;
    }
  s = ctts_block_tree_sum<LD_GATE_THREADS>(s, red);
  cnt = ctts_block_tree_sum<LD_GATE_THREADS>(cnt, red);
  double L = -INFINITY;
  if (cnt > 0.0) {
    const double gr = -0.691 + 10.0 * log10(s / cnt) - 10.0;
    s = 0.0;
    cnt = 0.0;
    for (int j = tid; j < nb; j += LD_GATE_THREADS) {
      const double l = -0.691 + 10.0 * log10(z[j]);
      if (l > gr && l > -70.0) {
        s += z[j];
        cnt += 1.0;
      }
    }
    s = ctts_block_tree_sum<LD_GATE_THREADS>(s, red);
    cnt = ctts_block_tree_sum<LD_GATE_THREADS>(cnt, red);
    if (cnt > 0.0) L = -0.691 + 10.0 * log10(s / cnt);
  }
  if (tid == 0) {
    const bool ok = L > -INFINITY && L < INFINITY;
    float g = 1.0f;
    if (ok) {
      const double gd = pow(10.0, (target - L) / 20.0);
      const float pk = peak[b];
      // peak guard: x g / max |x g| = x / max |x|; a correctly rounded 1 / peak keeps fl(peak g) <= 1
      g = (peak_limit && (double)pk * gd > 1.0) ? __fdiv_rn(1.0f, pk) : (float)gd;
    }
    loudness[b] = ok ? L : -INFINITY;
    gain[b] = g;
    valid[b] = ok ? 1 : 0;
  }
}

template <bool VEC>
__global__ __launch_bounds__(AG_THREADS) void apply_gain_kernel(const float* wav, const int32_t* __restrict__ lens,
                                                                const float* __restrict__ gain, float* out, int N) {
  const int b = blockIdx.y;
  const int len = min(max(lens[b], 0), N);
  const float g = gain[b];
  const long row = (long)b * N;
  if (VEC) {
    const int i = (blockIdx.x * AG_THREADS + threadIdx.x) * 4;
    if (i >= N) return;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < len) v = *reinterpret_cast<const float4*>(wav + row + i);
    v.x = i < len ? __fmul_rn(v.x, g) : 0.f;                        // a select, so what lies at or beyond len cannot leak
    v.y = i + 1 < len ? __fmul_rn(v.y, g) : 0.f;
    v.z = i + 2 < len ? __fmul_rn(v.z, g) : 0.f;
    v.w = i + 3 < len ? __fmul_rn(v.w, g) : 0.f;
    *reinterpret_cast<float4*>(out + row + i) = v;
  } else {
    const int i = blockIdx.x * AG_THREADS + threadIdx.x;
    if (i < N) out[row + i] = i < len ? __fmul_rn(wav[row + i], g) : 0.f;
  }
}

}  // namespace

extern "C" int ctts_loudness_chunk(void) { return LD_CHUNK; }
extern "C" int ctts_loudness_tile_slots(void) { return LD_SLOTS; }
extern "C" int ctts_loudness_coef_doubles(void) { return LD_COEF_DOUBLES; }
extern "C" int ctts_loudness_max_segments(void) { return LD_MAX_SEGS; }

extern "C" size_t ctts_loudness_workspace_bytes(int B, int N) {
  if (B < 1 || N < 1 || N > LD_MAX_N) return 0;
  return sizeof(double) * 4 * (size_t)ld_make_levels(N).stride * (size_t)B;
}

extern "C" int ctts_kweight_energy(const float* wav, const int32_t* lens, const double* coef, const int32_t* edges, const int32_t* chunk_seg,
                                   double* hop_sums, float* peak, int B, int N, int n_edges, int n_chunk_seg, void* workspace, void* stream) {
  CTTS_REQUIRE(wav && lens && coef && edges && chunk_seg && hop_sums && peak && workspace && B > 0 && N > 0, "ctts_kweight_energy: bad arguments");
  CTTS_REQUIRE(B <= 65535, "ctts_kweight_energy: at most 65535 utterances per call (got %d)", B);
  CTTS_REQUIRE(N <= LD_MAX_N, "ctts_kweight_energy: at most 2^24 samples per row (got %d)", N);
  const int nch = (N + LD_CHUNK - 1) / LD_CHUNK, ntiles = (N + LD_TILE - 1) / LD_TILE;
  CTTS_REQUIRE(n_edges >= 2 && n_chunk_seg >= ntiles * 64, "ctts_kweight_energy: the segment tables do not cover %d samples (%d chunks)", N, nch);
  hipStream_t st = (hipStream_t)stream;
  const ld_levels lv = ld_make_levels(N);
  if (ctts_zero_async(peak, sizeof(float) * (size_t)B, st) != 0) return -2;
  const dim3 grid(ntiles, B);
  if (nch > 1) {
    hipLaunchKernelGGL(kweight_kernel<false>, grid, dim3(64), 0, st, wav, lens, coef, edges, chunk_seg, (double*)workspace, hop_sums,
                       reinterpret_cast<unsigned*>(peak), N, n_edges, ntiles, lv.stride);
    CTTS_CHECK_LAUNCH("ctts_kweight_energy (zero-state pass)");
    hipLaunchKernelGGL(scan_kernel, dim3(B), dim3(256), 0, st, lens, coef, (double*)workspace, N, lv);
    CTTS_CHECK_LAUNCH("ctts_kweight_energy (state scan)");
  }
  hipLaunchKernelGGL(kweight_kernel<true>, grid, dim3(64), 0, st, wav, lens, coef, edges, chunk_seg, (double*)workspace, hop_sums,
                     reinterpret_cast<unsigned*>(peak), N, n_edges, ntiles, lv.stride);
  CTTS_CHECK_LAUNCH("ctts_kweight_energy");
  return 0;
}

extern "C" int ctts_loudness_gate(const double* hop_sums, const int32_t* lens, const int32_t* n_blocks, const int32_t* edges,
                                  const int32_t* chunk_seg, const int32_t* blocks, const float* peak, double* loudness, float* gain,
                                  int32_t* valid, double* curve, int B, int N, int n_edges, int n_chunk_seg, int J, double block_samples,
                                  double target, int peak_limit, void* stream) {
  CTTS_REQUIRE(hop_sums && lens && n_blocks && edges && chunk_seg && blocks && peak && loudness && gain && valid && B > 0 && N > 0,
               "ctts_loudness_gate: bad arguments");
  CTTS_REQUIRE(B <= 65535 && N <= LD_MAX_N, "ctts_loudness_gate: at most 65535 utterances of 2^24 samples (got %d x %d)", B, N);
  CTTS_REQUIRE(J >= 1 && J <= LD_MAX_SEGS && n_edges >= 2 && n_edges - 1 <= LD_MAX_SEGS + 1,
               "ctts_loudness_gate: at most %d blocks and hop segments per utterance (got %d / %d)", LD_MAX_SEGS, J, n_edges - 1);
  const int ntiles = (N + LD_TILE - 1) / LD_TILE;
  CTTS_REQUIRE(n_chunk_seg >= ntiles * 64, "ctts_loudness_gate: the segment tables do not cover %d samples", N);
  CTTS_REQUIRE(block_samples > 0.0 && target == target && target > -INFINITY && target < INFINITY,
               "ctts_loudness_gate: need a positive block length and a finite target");
  hipLaunchKernelGGL(gate_kernel, dim3(B), dim3(LD_GATE_THREADS), 0, (hipStream_t)stream, hop_sums, lens, n_blocks, edges, chunk_seg, blocks, peak,
                     loudness, gain, valid, curve, N, n_edges, J, ntiles, 1.0 / block_samples, target, peak_limit);
  CTTS_CHECK_LAUNCH("ctts_loudness_gate");
  return 0;
}

extern "C" int ctts_apply_gain(const float* wav, const int32_t* lens, const float* gain, float* out, int B, int N, void* stream) {
  CTTS_REQUIRE(wav && lens && gain && out && B > 0 && N > 0, "ctts_apply_gain: bad arguments");
  CTTS_REQUIRE(B <= 65535, "ctts_apply_gain: at most 65535 utterances per call (got %d)", B);
  hipStream_t st = (hipStream_t)stream;
  if (N % 4 == 0 && (((uintptr_t)wav | (uintptr_t)out) & 15) == 0) {
    hipLaunchKernelGGL(apply_gain_kernel<true>, dim3((N / 4 + AG_THREADS - 1) / AG_THREADS, B), dim3(AG_THREADS), 0, st, wav, lens, gain, out, N);
  } else {
    hipLaunchKernelGGL(apply_gain_kernel<false>, dim3((N + AG_THREADS - 1) / AG_THREADS, B), dim3(AG_THREADS), 0, st, wav, lens, gain, out, N);
  }
  CTTS_CHECK_LAUNCH("ctts_apply_gain");
  return 0;
}
