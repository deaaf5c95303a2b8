// Fastformer additive attention (reference: model/transformers/fastformer.py, wuch15's FastAttention): masked softmax pooling over
// time and the broadcast products around it, forward and backward.  Everything here streams [B*T, C] fp32 tensors once or twice, so the
// kernels are bound by HBM / L2 bytes, not arithmetic.  Layout: rows (b, t) over the PADDED length T, columns c = h*D + j (H heads of
// size D; the shipped config swaps the arguments and runs H = 128 heads of D = 2).  The logits s [B*T, H] come from the GEMMs.
//
// Reference semantics kept bit-for-bit where they are observable:
//   z = s / sqrt(D), then z + m with m = -10000 on VALID frames and 0 on padding (the mask polarity is inverted in the reference), in
//   fp32 and in that order - the add rounds z to the 2^-10 grid near -10000 on unpadded utterances, and padded rows dominate the pooling
//   of padded ones.  No row is skipped.
// Reductions over T run per 32-row chunk into a workspace and are combined in chunk order: no float atomics, bit-reproducible.
#include "ctts_common.h"

namespace {

constexpr int FF_TC = 32;         // rows per chunk of the reductions over T

__device__ __forceinline__ float ff_logit(float s, float div, int t, int len) {
  const float z = s / div;
  return z + (t < len ? -10000.0f : 0.0f);
}

// sum over the D lanes of one head (D a power of two <= 64: the lanes of a head are neighbours inside one wave)
__device__ __forceinline__ float ff_head_sum(float v, int D) {
  for (int o = 1; o < D; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// pass 1: per (b, chunk) and column: running max m, sum l = sum exp(z - m), acc = sum exp(z - m) V   (thread = column)
__global__ __launch_bounds__(1024) void ff_pool_part_kernel(const float* __restrict__ s, long lds, const float* __restrict__ V, long ldv,
                                                            const int32_t* __restrict__ lens, float* __restrict__ pm,
                                                            float* __restrict__ pl, float* __restrict__ pa, int T, int H, int C, int D,
                                                            float div) {
  const int ch = blockIdx.x, b = blockIdx.y, c = threadIdx.x, h = c / D, nch = gridDim.x;
  const int t0 = ch * FF_TC, t1 = min(T, t0 + FF_TC);
  const int len = lens[b];
  float m = -INFINITY, l = 0.0f, a = 0.0f;
  for (int t = t0; t < t1; ++t) {
    const long r = (long)b * T + t;
    const float z = ff_logit(s[r * lds + h], div, t, len);
    const float v = V[r * ldv + c];
    if (z > m) {
      const float sc = expf(m - z);
      l *= sc; a *= sc; m = z;
    }
    const float e = expf(z - m);
    l += e;
    a += e * v;
  }
  const long o = (long)b * nch + ch;
  pa[o * C + c] = a;
  if (c % D == 0) { pm[o * H + h] = m; pl[o * H + h] = l; }
}

// pass 2: p[b, c] = sum_chunks acc exp(m - M) / L,  stats[b, h] = (M, L)   (chunk order fixed)
__global__ __launch_bounds__(1024) void ff_pool_combine_kernel(const float* __restrict__ pm, const float* __restrict__ pl,
                                                               const float* __restrict__ pa, float* __restrict__ p,
                                                               float* __restrict__ stats, int nch, int H, int C, int D) {
  const int b = blockIdx.x, c = threadIdx.x, h = c / D;
  float M = -INFINITY;
  for (int k = 0; k < nch; ++k) M = fmaxf(M, pm[((long)b * nch + k) * H + h]);
  float L = 0.0f, A = 0.0f;
  for (int k = 0; k < nch; ++k) {
    const long o = (long)b * nch + k;
    const float w = expf(pm[o * H + h] - M);
    L += pl[o * H + h] * w;
    A += pa[o * C + c] * w;
  }
  p[(long)b * C + c] = A / L;
  if (c % D == 0) { stats[((long)b * H + h) * 2] = M; stats[((long)b * H + h) * 2 + 1] = L; }
}

// alpha = exp(z - M) / L;  dV = dVin + alpha dp;  ds = alpha (sum_j V dp - sum_j p dp) / sqrt(D)
__global__ __launch_bounds__(1024) void ff_pool_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ p,
                                                           const float* __restrict__ stats, const float* __restrict__ s, long lds,
                                                           const float* __restrict__ V, long ldv, const int32_t* __restrict__ lens,
                                                           const float* dVin, float* dV, float* __restrict__ ds, int T, int H, int C,
                                                           int D, float div) {
  const int ch = blockIdx.x, b = blockIdx.y, c = threadIdx.x, h = c / D;
  const int t0 = ch * FF_TC, t1 = min(T, t0 + FF_TC);
  const int len = lens[b];
  const float M = stats[((long)b * H + h) * 2], L = stats[((long)b * H + h) * 2 + 1];
  const float dpc = dp[(long)b * C + c];
  const float pdp = ff_head_sum(p[(long)b * C + c] * dpc, D);
  for (int t = t0; t < t1; ++t) {
    const long r = (long)b * T + t;
    const float alpha = expf(ff_logit(s[r * lds + h], div, t, len) - M) / L;
    const float g = ff_head_sum(V[r * ldv + c] * dpc, D);
    dV[r * C + c] = (dVin ? dVin[r * C + c] : 0.0f) + alpha * dpc;
    if (c % D == 0) ds[r * H + h] = alpha * (g - pdp) / div;
  }
}

// Y[b, t, :] = X[b, t, :] * p[b, :]
__global__ void ff_bcast_kernel(const float4* __restrict__ X, long ldx4, const float4* __restrict__ p, float4* __restrict__ Y, long rows,
                                int T, int C4) {
  const long total = rows * C4;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long r = e / C4; const int c = (int)(e - r * C4);
    const long b = r / T;
    const float4 x = X[r * ldx4 + c], q = p[b * C4 + c];
    Y[e] = make_float4(x.x * q.x, x.y * q.y, x.z * q.z, x.w * q.w);
  }
}

// dy = dY1 (+ dY2);  dX = dXin + dy p[b];  part[b, chunk, c] = sum_t dy X
__global__ __launch_bounds__(1024) void ff_bcast_bwd_kernel(const float* __restrict__ dY1, const float* __restrict__ dY2,
                                                            const float* __restrict__ X, long ldx, const float* __restrict__ p,
                                                            const float* dXin, float* dX, float* __restrict__ part, int T, int C) {
  const int ch = blockIdx.x, b = blockIdx.y, c = threadIdx.x, nch = gridDim.x;
  const int t0 = ch * FF_TC, t1 = min(T, t0 + FF_TC);
  const float pc = p[(long)b * C + c];
  float acc = 0.0f;
  for (int t = t0; t < t1; ++t) {
    const long r = (long)b * T + t;
    const float dy = dY1[r * C + c] + (dY2 ? dY2[r * C + c] : 0.0f);
    dX[r * C + c] = (dXin ? dXin[r * C + c] : 0.0f) + dy * pc;
    acc += dy * X[r * ldx + c];
  }
  part[((long)b * nch + ch) * C + c] = acc;
}

__global__ __launch_bounds__(1024) void ff_colsum_chunks_kernel(const float* __restrict__ part, float* __restrict__ out, int nch, int C) {
  const int b = blockIdx.x, c = threadIdx.x;
  float acc = 0.0f;
  for (int k = 0; k < nch; ++k) acc += part[((long)b * nch + k) * C + c];
  out[(long)b * C + c] = acc;
}

// y = rowscale * (x + drop(t))        backward: dt = rowscale * drop(dy), dx = rowscale * dy
__global__ void ff_resdrop_kernel(const float4* __restrict__ x, const float4* __restrict__ t, float4* __restrict__ y,
                                  float4* __restrict__ y2, long rows, int C4, const float* __restrict__ rowscale, float p,
                                  const uint64_t* __restrict__ seed, uint32_t off, int backward) {
  const long total = rows * C4;
  const uint32_t key = ctts_drop_key(seed, off);
  const float inv_keep = p > 0.0f ? 1.0f / (1.0f - p) : 1.0f;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long r = e / C4;
    const float rs = rowscale ? rowscale[r] : 1.0f;
    const float4 v = t[e];
    float d[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (p > 0.0f) {
      const uint32_t i0 = (uint32_t)(e * 4);
      for (int k = 0; k < 4; ++k) d[k] = ctts_drop_scale(key, i0 + k, p, inv_keep);
    }
    const float4 dv = make_float4(rs * (v.x * d[0]), rs * (v.y * d[1]), rs * (v.z * d[2]), rs * (v.w * d[3]));
    if (backward) {
      y[e] = dv;
      y2[e] = make_float4(rs * v.x, rs * v.y, rs * v.z, rs * v.w);
    } else {
      const float4 a = x[e];
      y[e] = make_float4(rs * (a.x + v.x * d[0]), rs * (a.y + v.y * d[1]), rs * (a.z + v.z * d[2]), rs * (a.w + v.w * d[3]));
    }
  }
}

inline int grid_for(long n, int cap = 8192) { return (int)min((n + 255) / 256, (long)cap); }

bool ff_shape_ok(int H, int C, int D) {
  return H > 0 && D > 0 && (D & (D - 1)) == 0 && D <= 64 && H * D == C && C % 64 == 0 && C <= 1024;
}

}  // namespace

extern "C" size_t ctts_fastformer_workspace_floats(int B, int T, int H, int C) {
  if (B <= 0 || T <= 0) return 0;
  return (size_t)B * ((T + FF_TC - 1) / FF_TC) * (2 * (size_t)H + C);
}

extern "C" int ctts_fastformer_pool_fwd(const float* s, int64_t lds, const float* V, int64_t ldv, const int32_t* lens, float* p,
                                        float* stats, float* ws, int B, int T, int H, int C, float div, void* stream) {
  CTTS_REQUIRE(s && V && lens && p && stats && ws && B >= 0 && T >= 0 && ff_shape_ok(H, C, C / (H > 0 ? H : 1)) && lds >= H && ldv >= C &&
                   div > 0.0f,
               "ctts_fastformer_pool_fwd: bad arguments (need H*D == C, D a power of two <= 64, C %% 64 == 0, C <= 1024)");
  if (B == 0) return 0;
  CTTS_REQUIRE(T > 0, "ctts_fastformer_pool_fwd: T must be >= 1 (softmax over an empty sequence)");
  const int D = C / H, nch = (T + FF_TC - 1) / FF_TC;
  float* pm = ws;
  float* pl = pm + (size_t)B * nch * H;
  float* pa = pl + (size_t)B * nch * H;
  hipLaunchKernelGGL(ff_pool_part_kernel, dim3(nch, B), dim3(C), 0, (hipStream_t)stream, s, (long)lds, V, (long)ldv, lens, pm, pl, pa, T,
                     H, C, D, div);
  CTTS_CHECK_LAUNCH("ctts_fastformer_pool_fwd (part)");
  hipLaunchKernelGGL(ff_pool_combine_kernel, dim3(B), dim3(C), 0, (hipStream_t)stream, pm, pl, pa, p, stats, nch, H, C, D);
  CTTS_CHECK_LAUNCH("ctts_fastformer_pool_fwd (combine)");
  return 0;
}

extern "C" int ctts_fastformer_pool_bwd(const float* dp, const float* p, const float* stats, const float* s, int64_t lds, const float* V,
                                        int64_t ldv, const int32_t* lens, const float* dV_in, float* dV, float* ds, int B, int T, int H,
                                        int C, float div, void* stream) {
  CTTS_REQUIRE(dp && p && stats && s && V && lens && dV && ds && B >= 0 && T >= 0 && ff_shape_ok(H, C, C / (H > 0 ? H : 1)) &&
                   lds >= H && ldv >= C && div > 0.0f,
               "ctts_fastformer_pool_bwd: bad arguments (need H*D == C, D a power of two <= 64, C %% 64 == 0, C <= 1024)");
  if (B == 0 || T == 0) return 0;
  const int D = C / H, nch = (T + FF_TC - 1) / FF_TC;
  hipLaunchKernelGGL(ff_pool_bwd_kernel, dim3(nch, B), dim3(C), 0, (hipStream_t)stream, dp, p, stats, s, (long)lds, V, (long)ldv, lens,
                     dV_in, dV, ds, T, H, C, D, div);
  CTTS_CHECK_LAUNCH("ctts_fastformer_pool_bwd");
  return 0;
}

extern "C" int ctts_fastformer_bcast(const float* X, int64_t ldx, const float* p, float* Y, int B, int T, int C, void* stream) {
  CTTS_REQUIRE(X && p && Y && B >= 0 && T >= 0 && C > 0 && C % 4 == 0 && ldx >= C && ldx % 4 == 0 &&
                   ((uintptr_t)X % 16) == 0 && ((uintptr_t)p % 16) == 0 && ((uintptr_t)Y % 16) == 0,
               "ctts_fastformer_bcast: bad arguments (C and ldx multiples of 4, 16-byte aligned)");
  const long rows = (long)B * T;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(ff_bcast_kernel, dim3(grid_for(rows * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(X), (long)(ldx / 4), reinterpret_cast<const float4*>(p), reinterpret_cast<float4*>(Y),
                     rows, T, C / 4);
  CTTS_CHECK_LAUNCH("ctts_fastformer_bcast");
  return 0;
}

extern "C" int ctts_fastformer_bcast_bwd(const float* dY1, const float* dY2, const float* X, int64_t ldx, const float* p,
                                         const float* dX_in, float* dX, float* dp, float* ws, int B, int T, int C, void* stream) {
  CTTS_REQUIRE(dY1 && X && p && dX && dp && ws && B >= 0 && T >= 0 && C > 0 && C % 64 == 0 && C <= 1024 && ldx >= C,
               "ctts_fastformer_bcast_bwd: bad arguments (C %% 64 == 0, C <= 1024)");
  if (B == 0) return 0;
  const int nch = (T + FF_TC - 1) / FF_TC;
  if (nch > 0) {
    hipLaunchKernelGGL(ff_bcast_bwd_kernel, dim3(nch, B), dim3(C), 0, (hipStream_t)stream, dY1, dY2, X, (long)ldx, p, dX_in, dX, ws, T, C);
    CTTS_CHECK_LAUNCH("ctts_fastformer_bcast_bwd (part)");
  }
  hipLaunchKernelGGL(ff_colsum_chunks_kernel, dim3(B), dim3(C), 0, (hipStream_t)stream, ws, dp, nch, C);
  CTTS_CHECK_LAUNCH("ctts_fastformer_bcast_bwd (combine)");
  return 0;
}

extern "C" int ctts_fastformer_resdrop(const float* x, const float* t, float* y, float* y2, int64_t rows, int C, const float* rowscale,
                                       float p_drop, const uint64_t* seed, uint32_t drop_offset, int backward, void* stream) {
  CTTS_REQUIRE(t && y && (backward ? y2 != nullptr : x != nullptr) && C > 0 && C % 4 == 0 && p_drop >= 0.0f && p_drop < 1.0f,
               "ctts_fastformer_resdrop: bad arguments (C %% 4 must be 0, 0 <= p < 1)");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(ff_resdrop_kernel, dim3(grid_for((long)rows * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(t), reinterpret_cast<float4*>(y),
                     reinterpret_cast<float4*>(y2), (long)rows, C / 4, rowscale, p_drop, seed, drop_offset, backward);
  CTTS_CHECK_LAUNCH("ctts_fastformer_resdrop");
  return 0;
}
