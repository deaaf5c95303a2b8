// Objective evaluation on the device: how close a synthesised utterance is to its recording.
//  * ctts_mel_cepstrum : log-mel [B,M,F] -> cepstra [B,F,K], the orthonormal DCT-II over the mel axis without coefficient 0.
//  * ctts_dtw          : dynamic time warping of two cepstral sequences per pair: a tiled launch forms the local costs (Euclidean
//                        distances, all pairs and tiles in parallel, stored one anti-diagonal per row), then ONE workgroup per pair sweeps the anti-diagonals of the DP
//                        (the recurrence needs the cell to the left in the same row, so a row cannot be relaxed in parallel the way
//                        mas_kernel of align.hip does it), records two direction bits per cell and walks the path back.
//  * ctts_path_metrics : counts and the squared log-F0 distance (cents) over the aligned frame pairs, ordered reduction in double.
// Lengths are int32 device arrays, read once per workgroup and clamped to the padded sizes; rows at or beyond a length are never read
// (they may hold NaN).  No float atomics: every sum has one fixed order, results are bit-identical run to run.
#include "ctts_common.h"

namespace {

constexpr int MC_MAX_K = 32;         // cepstral coefficients kept in registers
constexpr int DTW_MAX_T = 2048;      // padded frames per side
constexpr int DTW_THREADS = 256;
constexpr int DTW_CH = 8;            // anti-diagonals per chunk: one 16-bit direction word per (chunk, row), costs prefetched one chunk ahead

// ---------------------------------------------------------------------------------------------------------------- mel cepstrum
// One thread per frame; the table sqrt(2/M) cos(pi k (m + 1/2) / M) in LDS (every lane reads the same entry: a broadcast), the mel
// read channel by channel (lanes = consecutive frames of one channel row: coalesced), the M terms added in channel order.
__global__ __launch_bounds__(256) void mel_cepstrum_kernel(const float* __restrict__ mel, const int* __restrict__ frames,
                                                            float* __restrict__ out, int M, int F, int K) {
  extern __shared__ float s_dct[];                 // [M][K]
  const int b = blockIdx.y;
  const double scale = sqrt(2.0 / (double)M);
  for (int e = threadIdx.x; e < M * K; e += 256) {
    const int m = e / K, k = e - m * K + 1;
    const int q = (int)(((long)k * (2 * m + 1)) % (4L * M));           // the angle pi k (2m + 1) / (2M), reduced exactly
    s_dct[e] = (float)(scale * cospi((double)q / (2.0 * (double)M)));
  }
  __syncthreads();
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const int nf = frames ? min(max(frames[b], 0), F) : F;
  float acc[MC_MAX_K];
#pragma unroll
  for (int k = 0; k < MC_MAX_K; ++k) acc[k] = 0.f;
  if (f < nf) {
    const float* src = mel + (long)b * M * F + f;
    for (int m = 0; m < M; ++m) {
      const float v = src[(long)m * F];
#pragma unroll
      for (int k = 0; k < MC_MAX_K; ++k)
        if (k < K) acc[k] = fmaf(v, s_dct[m * K + k], acc[k]);
    }
  }
  float* dst = out + ((long)b * F + f) * K;
#pragma unroll
  for (int k = 0; k < MC_MAX_K; ++k)
    if (k < K) dst[k] = acc[k];
}

// ---------------------------------------------------------------------------------------------------------------- DTW: local costs
// d(i,j) = ||x_i - y_j||_2 for i < Lx, j < Ly, stored SKEWED: S[b][i + j][i], one row of `ld` floats per anti-diagonal, so that the
// sweep - whose threads own rows and walk the anti-diagonals - reads consecutive floats from consecutive lanes.  (Row-major costs made
// every lane of the sweep touch a cache line of its own: 2048 line requests per wave and 8 diagonals, and the sweep ran at the rate of
// those requests.)  Nothing outside Lx x Ly is written, and the sweep uses nothing else.  64 x 64 tile, both operands' rows in LDS,
// lane -> x row, wave -> every fourth anti-diagonal of the tile: the stores of a wave are 256 contiguous bytes.
__global__ __launch_bounds__(256) void dtw_cost_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        const int* __restrict__ x_lens, const int* __restrict__ y_lens,
                                                        float* __restrict__ S, int Tx, int Ty, int K, int ld) {
  __shared__ float s_x[64][MC_MAX_K + 1], s_y[64][MC_MAX_K + 1];
  const int b = blockIdx.z;
  const int Lx = min(max(x_lens[b], 0), Tx), Ly = min(max(y_lens[b], 0), Ty);
  const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
  if (i0 >= Lx || j0 >= Ly) return;                 // workgroup-uniform, before the barrier
  for (int e = threadIdx.x; e < 64 * K; e += 256) {
    const int s = e / K, c = e - s * K;
    s_x[s][c] = (i0 + s < Lx) ? x[((long)b * Tx + i0 + s) * K + c] : 0.f;
    s_y[s][c] = (j0 + s < Ly) ? y[((long)b * Ty + j0 + s) * K + c] : 0.f;
  }
  __syncthreads();
  const int il = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* Sb = S + (long)b * (Tx + Ty - 1) * ld;
  const bool row_ok = i0 + il < Lx;
  for (int dl = w; dl < 127; dl += 4) {
    const int jl = dl - il;
    if (row_ok && jl >= 0 && jl < 64 && j0 + jl < Ly) {
      float acc = 0.f;
      for (int c = 0; c < K; ++c) {
        const float d = s_x[il][c] - s_y[jl][c];
        acc = fmaf(d, d, acc);
      }
      Sb[(long)(i0 + j0 + dl) * ld + i0 + il] = sqrtf(acc);
    }
  }
}

// NR consecutive floats from an address aligned to 4 NR bytes
template <int NR>
__device__ __forceinline__ void dtw_load_row(const float* __restrict__ p, float (&v)[NR]) {
  if constexpr (NR == 1) {
    v[0] = p[0];
  } else if constexpr (NR == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  } else {
#pragma unroll
    for (int k = 0; k < NR / 4; ++k) {
      const float4 t = reinterpret_cast<const float4*>(p)[k];
      v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- DTW: sweep + backtrack
// One workgroup per pair.  Thread t owns the NR consecutive rows t NR .. t NR + NR - 1; on anti-diagonal d it relaxes the cells
// (i, d - i) of its rows.  The two previous diagonals of its own rows stay in registers; the only value that crosses threads is the
// last row of thread t - 1, handed over through a double-buffered LDS word per thread: one barrier per diagonal, and the number of
// diagonals, Lx + Ly - 1, is the same for every thread of the workgroup.  A cell outside Lx x Ly holds +inf and its cost is never
// used; a predecessor that does not exist is therefore +inf and cannot win (A(-1,-1) = 0 in front of cell (0,0)).  Direction of a cell: 0 = (i-1, j-1), 1 = (i-1, j), 2 = (i, j-1);
// the diagonal wins when it is <= both others, then (i-1, j), then (i, j-1).  Two bits per cell: the 8 diagonals of a chunk make one
// 16-bit word per row, stored at dirs[chunk][row] (consecutive lanes, rows NR apart).
template <int NR>
__global__ __launch_bounds__(DTW_THREADS) void dtw_sweep_kernel(const float* __restrict__ S, const int* __restrict__ x_lens,
                                                                 const int* __restrict__ y_lens, unsigned short* __restrict__ dirs,
                                                                 float* __restrict__ cost, int* __restrict__ path_len,
                                                                 int* __restrict__ path, int Tx, int Ty, int ld) {
  __shared__ float s_edge[2][DTW_THREADS];
  __shared__ short s_path[2 * DTW_MAX_T][2];       // the path as the backtrack meets it: last pair first
  __shared__ int s_len;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Lx = min(max(x_lens[b], 0), Tx), Ly = min(max(y_lens[b], 0), Ty);      // read once
  const int P = Tx + Ty - 1;
  int* pth = path + (long)b * P * 2;
  if (Lx == 0 || Ly == 0) {                         // workgroup-uniform exit before the first barrier
    for (int e = tid; e < 2 * P; e += DTW_THREADS) pth[e] = -1;
    if (tid == 0) { cost[b] = 0.f; path_len[b] = 0; }
    return;
  }
  const int ndiag = Lx + Ly - 1;
  const int nchunk = (Tx + Ty - 1 + DTW_CH - 1) / DTW_CH;
  const float* Sb = S + (long)b * P * ld;           // skewed costs: row d holds d(i, d - i) at column i
  unsigned short* dirb = dirs + (long)b * nchunk * Tx;
  const int row0 = tid * NR;

  float nx[NR][DTW_CH];
  auto load_chunk = [&](int d0) {                   // one aligned vector load per diagonal; what lies outside Lx x Ly is dropped unused
#pragma unroll
    for (int q = 0; q < DTW_CH; ++q) {
      const int d = d0 + q;
      float v[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) v[r] = 0.f;
      if (row0 < Lx && d < ndiag) dtw_load_row<NR>(Sb + (long)d * ld + row0, v);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int i = row0 + r, j = d - i;
        nx[r][q] = (i < Lx && j >= 0 && j < Ly) ? v[r] : 0.f;
      }
    }
  };
  float p1[NR], p2[NR];                             // A on diagonals d - 1 and d - 2, own rows
#pragma unroll
  for (int r = 0; r < NR; ++r) p1[r] = p2[r] = INFINITY;
  // the same for row row0 - 1 (thread tid - 1); thread 0 starts from A(-1,-1) = 0, the diagonal predecessor of cell (0,0)
  float e1 = tid == 0 ? 0.f : INFINITY, e2 = INFINITY;
  int dlo[NR], dhi[NR];                             // row i holds a cell on diagonal d iff i <= d <= i + Ly - 1 (and i < Lx)
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    dlo[r] = row0 + r < Lx ? row0 + r : 0x7fffffff;
    dhi[r] = row0 + r + Ly - 1;
  }
  s_edge[0][tid] = INFINITY;
  s_edge[1][tid] = INFINITY;
  load_chunk(0);
  __syncthreads();
  for (int d0 = 0; d0 < ndiag; d0 += DTW_CH) {
    float cst[NR][DTW_CH];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int q = 0; q < DTW_CH; ++q) cst[r][q] = nx[r][q];
    if (d0 + DTW_CH < ndiag) load_chunk(d0 + DTW_CH);                 // in flight while this chunk's 8 diagonals run
    unsigned word[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) word[r] = 0u;
#pragma unroll
    for (int q = 0; q < DTW_CH; ++q) {
      const int d = d0 + q;
      if (d >= ndiag) break;                        // ndiag is workgroup-uniform: so is this exit
      e2 = e1;
      e1 = tid > 0 ? s_edge[(d + 1) & 1][tid - 1] : INFINITY;         // written on diagonal d - 1
      float cur[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) {                // branch-free: a predecessor that does not exist is +inf by construction
        const float up = r == 0 ? e1 : p1[r - 1], dg = r == 0 ? e2 : p2[r - 1], left = p1[r];
        float best = dg;
        unsigned dir = 0u;
        if (up < best) { best = up; dir = 1u; }
        if (left < best) { best = left; dir = 2u; }
        cur[r] = (d >= dlo[r] && d <= dhi[r]) ? cst[r][q] + best : INFINITY;
        word[r] |= dir << (2 * q);                  // bits of a cell outside Lx x Ly are never looked at
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) { p2[r] = p1[r]; p1[r] = cur[r]; }
      s_edge[d & 1][tid] = cur[NR - 1];
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (row0 + r < Lx) dirb[(long)(d0 / DTW_CH) * Tx + row0 + r] = (unsigned short)word[r];
  }
  // p1 holds the last diagonal: its only cell is (Lx - 1, Ly - 1)
#pragma unroll
  for (int r = 0; r < NR; ++r)
    if (row0 + r == Lx - 1) cost[b] = p1[r];
  __syncthreads();                                  // the direction words of every thread are visible to the walker
  if (tid == 0) {
    int i = Lx - 1, j = Ly - 1, n = 0;
    for (; n < ndiag; ++n) {                        // a path has at most Lx + Ly - 1 pairs
      s_path[n][0] = (short)i;
      s_path[n][1] = (short)j;
      if (i == 0 && j == 0) { ++n; break; }
      const int d = i + j;
      unsigned dir = (dirb[(long)(d / DTW_CH) * Tx + i] >> (2 * (d % DTW_CH))) & 3u;
      if (i == 0) dir = 2u;                         // what the sweep recorded there anyway: keeps the walk inside whatever it reads
      else if (j == 0) dir = 1u;
      if (dir != 2u) --i;
      if (dir != 1u) --j;
    }
    s_len = n;
    path_len[b] = n;
  }
  __syncthreads();
  const int n = s_len;
  for (int e = tid; e < P; e += DTW_THREADS) {
    pth[2 * e] = e < n ? (int)s_path[n - 1 - e][0] : -1;
    pth[2 * e + 1] = e < n ? (int)s_path[n - 1 - e][1] : -1;
  }
}

// align = none: frame i against frame i over min(Lx, Ly) frames; the same outputs as the sweep, the cost summed in one fixed order
// (per thread over its frames i = tid, tid + 256, ..., then a tree over the threads).
__global__ __launch_bounds__(DTW_THREADS) void dtw_identity_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                    const int* __restrict__ x_lens, const int* __restrict__ y_lens,
                                                                    float* __restrict__ cost, int* __restrict__ path_len,
                                                                    int* __restrict__ path, int Tx, int Ty, int K) {
  __shared__ float s_sum[DTW_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Lx = min(max(x_lens[b], 0), Tx), Ly = min(max(y_lens[b], 0), Ty);
  const int n = min(Lx, Ly), P = Tx + Ty - 1;
  int* pth = path + (long)b * P * 2;
  float s = 0.f;
  for (int i = tid; i < n; i += DTW_THREADS) {
    const float* xr = x + ((long)b * Tx + i) * K;
    const float* yr = y + ((long)b * Ty + i) * K;
    float acc = 0.f;
    for (int c = 0; c < K; ++c) {
      const float d = xr[c] - yr[c];
      acc = fmaf(d, d, acc);
    }
    s += sqrtf(acc);
  }
  s_sum[tid] = s;
  __syncthreads();
  for (int w = DTW_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) s_sum[tid] += s_sum[tid + w];
    __syncthreads();
  }
  for (int e = tid; e < P; e += DTW_THREADS) pth[2 * e] = pth[2 * e + 1] = e < n ? e : -1;
  if (tid == 0) { cost[b] = s_sum[0]; path_len[b] = n; }
}

// ---------------------------------------------------------------------------------------------------------------- path metrics
// out[b] = (pairs, pairs voiced in both, sum over those of (1200 log2(f0_x / f0_y))^2, pairs whose voicing differs) in double.
// Per thread over its pairs p = tid, tid + 256, ... in order, then a tree over the threads: one fixed order.
__global__ __launch_bounds__(256) void path_metrics_kernel(const int* __restrict__ path, const int* __restrict__ path_len,
                                                            const float* __restrict__ f0_x, const float* __restrict__ f0_y,
                                                            double* __restrict__ out, int Tx, int Ty, int P) {
  __shared__ double s_sq[256];
  __shared__ int s_cnt[3][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(path_len[b], 0), P);
  const int* pth = path + (long)b * P * 2;
  int pairs = 0, both = 0, differ = 0;
  double sq = 0.0;
  for (int p = tid; p < n; p += 256) {
    const int i = pth[2 * p], j = pth[2 * p + 1];
    if (i < 0 || i >= Tx || j < 0 || j >= Ty) continue;               // not a pair: a caller's -1 padding inside path_len
    const float fx = f0_x[(long)b * Tx + i], fy = f0_y[(long)b * Ty + j];
    const bool vx = fx > 0.f, vy = fy > 0.f;
    ++pairs;
    if (vx && vy) {
      ++both;
      const double c = 1200.0 * log2((double)fx / (double)fy);
      sq += c * c;
    } else if (vx != vy) {
      ++differ;
    }
  }
  s_sq[tid] = sq;
  s_cnt[0][tid] = pairs;
  s_cnt[1][tid] = both;
  s_cnt[2][tid] = differ;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      s_sq[tid] += s_sq[tid + w];
      s_cnt[0][tid] += s_cnt[0][tid + w];
      s_cnt[1][tid] += s_cnt[1][tid + w];
      s_cnt[2][tid] += s_cnt[2][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[4 * b] = (double)s_cnt[0][0];
    out[4 * b + 1] = (double)s_cnt[1][0];
    out[4 * b + 2] = s_sq[0];
    out[4 * b + 3] = (double)s_cnt[2][0];
  }
}

int dtw_ld(int Tx) { return (Tx + 7) / 8 * 8; }      // floats per anti-diagonal row of the skewed costs: keeps every vector load aligned
size_t dtw_cost_bytes(int B, int Tx, int Ty) { return (size_t)B * (Tx + Ty - 1) * dtw_ld(Tx) * sizeof(float); }
size_t dtw_dir_bytes(int B, int Tx, int Ty) {
  return ((size_t)B * ((Tx + Ty - 1 + DTW_CH - 1) / DTW_CH) * Tx * sizeof(unsigned short) + 15) / 16 * 16;
}

}  // namespace

extern "C" int ctts_mel_cepstrum(const float* mel, const int32_t* frames, float* out, int B, int n_mel, int F, int n_coef, void* stream) {
  CTTS_REQUIRE(mel && out, "ctts_mel_cepstrum: null pointer");
  CTTS_REQUIRE(n_coef >= 1 && n_coef <= MC_MAX_K && n_coef < n_mel, "ctts_mel_cepstrum: need 1 <= n_coef <= %d and n_coef < n_mel, got %d / %d",
               MC_MAX_K, n_coef, n_mel);
  CTTS_REQUIRE((size_t)n_mel * n_coef * sizeof(float) <= 48 * 1024, "ctts_mel_cepstrum: n_mel=%d x n_coef=%d beyond the LDS table", n_mel, n_coef);
  CTTS_REQUIRE(B >= 0 && B <= 65535 && F >= 0, "ctts_mel_cepstrum: bad sizes B=%d F=%d", B, F);
  if (B == 0 || F == 0) return 0;
  hipLaunchKernelGGL(mel_cepstrum_kernel, dim3((F + 255) / 256, B), dim3(256), (size_t)n_mel * n_coef * sizeof(float), (hipStream_t)stream,
                     mel, frames, out, n_mel, F, n_coef);
  CTTS_CHECK_LAUNCH("ctts_mel_cepstrum");
  return 0;
}

extern "C" size_t ctts_dtw_workspace_bytes(int B, int Tx, int Ty) {
  if (B <= 0 || Tx <= 0 || Ty <= 0) return 0;
  return dtw_cost_bytes(B, Tx, Ty) + dtw_dir_bytes(B, Tx, Ty);
}

extern "C" int ctts_dtw(const float* x, const float* y, const int32_t* x_lens, const int32_t* y_lens, void* workspace, float* cost,
                        int32_t* path_len, int32_t* path, int B, int Tx, int Ty, int K, int align, void* stream) {
  CTTS_REQUIRE(Tx >= 1 && Ty >= 1 && Tx <= DTW_MAX_T && Ty <= DTW_MAX_T, "ctts_dtw: padded sizes %d x %d outside [1, %d]", Tx, Ty, DTW_MAX_T);
  CTTS_REQUIRE(K >= 1 && K <= MC_MAX_K, "ctts_dtw: K=%d outside [1, %d]", K, MC_MAX_K);
  CTTS_REQUIRE(B >= 0 && B <= 65535, "ctts_dtw: B=%d outside [0, 65535]", B);
  CTTS_REQUIRE(align == 0 || align == 1, "ctts_dtw: align must be 0 (dtw) or 1 (none), got %d", align);
  CTTS_REQUIRE(x && y && x_lens && y_lens && cost && path_len && path && (align == 1 || workspace), "ctts_dtw: null pointer");
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (align == 1) {
    hipLaunchKernelGGL(dtw_identity_kernel, dim3(B), dim3(DTW_THREADS), 0, st, x, y, x_lens, y_lens, cost, path_len, path, Tx, Ty, K);
    CTTS_CHECK_LAUNCH("ctts_dtw");
    return 0;
  }
  CTTS_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 32 == 0, "ctts_dtw: the workspace must be 32-byte aligned");
  float* D = reinterpret_cast<float*>(workspace);
  const int ld = dtw_ld(Tx);
  unsigned short* dirs = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(workspace) + dtw_cost_bytes(B, Tx, Ty));
  hipLaunchKernelGGL(dtw_cost_kernel, dim3((Tx + 63) / 64, (Ty + 63) / 64, B), dim3(256), 0, st, x, y, x_lens, y_lens, D, Tx, Ty, K, ld);
  CTTS_CHECK_LAUNCH("ctts_dtw");
  const int nr = (Tx + DTW_THREADS - 1) / DTW_THREADS;        // rows per thread: 1, 2, 4 or 8
#define CTTS_DTW_SWEEP(NR) \
  hipLaunchKernelGGL((dtw_sweep_kernel<NR>), dim3(B), dim3(DTW_THREADS), 0, st, D, x_lens, y_lens, dirs, cost, path_len, path, Tx, Ty, ld)
  if (nr <= 1) CTTS_DTW_SWEEP(1);
  else if (nr <= 2) CTTS_DTW_SWEEP(2);
  else if (nr <= 4) CTTS_DTW_SWEEP(4);
  else CTTS_DTW_SWEEP(8);
#undef CTTS_DTW_SWEEP
  CTTS_CHECK_LAUNCH("ctts_dtw");
  return 0;
}

extern "C" int ctts_path_metrics(const int32_t* path, const int32_t* path_len, const float* f0_x, const float* f0_y, double* out, int B,
                                 int Tx, int Ty, int P, void* stream) {
  CTTS_REQUIRE(path && path_len && f0_x && f0_y && out, "ctts_path_metrics: null pointer");
  CTTS_REQUIRE(B >= 0 && B <= 65535 && Tx >= 1 && Ty >= 1 && P >= 1, "ctts_path_metrics: bad sizes B=%d Tx=%d Ty=%d P=%d", B, Tx, Ty, P);
  if (B == 0) return 0;
  hipLaunchKernelGGL(path_metrics_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, path, path_len, f0_x, f0_y, out, Tx, Ty, P);
  CTTS_CHECK_LAUNCH("ctts_path_metrics");
  return 0;
}
