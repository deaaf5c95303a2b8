// Waveform metrics on the device (include/ctts.h "Waveform metrics on the device"): STOI / ESTOI, SI-SDR and the
// multi-resolution STFT distances of a synthesised utterance against its sample-aligned recording.  The definitions are those of
// ctts_amd.metrics (module docstring) and tests/wavmetrics_restate.py.
//
// The samples are fp32 and enter exactly; every product, transform and sum below is DOUBLE.  The work is small (a 60 s utterance is 4687
// STOI frames) and the MI355X runs fp64 vector arithmetic at half its fp32 rate, so the kernels sit three orders of magnitude under
// the float32 evaluation of the same chain instead of beside it, and the keep decision of the silent-frame step is the restatement's.
//   frame_spectrum<NFFT, EPI>  one workgroup per frame pair: both signals are windowed, packed as x + i y into ONE complex FFT of NFFT points
//                          in LDS (radix 2, decimation in time: fft_common.h) and unpacked by the Hermitian symmetry (in double the cross-talk of the
//                          packing is 2^-53 of the larger spectrum).  EPI_STOI gathers the frame through the kept-index list - the
//                          compacted signals never exist - and writes the 15 third-octave band amplitudes of both signals; EPI_MR takes
//                          frame i at i hop and writes the frame's four partial sums of the Parallel-WaveGAN distances.
//   st_energy_kernel       sum (w x)^2 of every 256-sample frame of the reference, one wave per frame
//   st_keep_kernel         one workgroup per utterance: the largest frame energy, the keep flags, their prefix sum -> kept-index list
//   st_segment_kernel      one wave per 15 x 30 segment: the STOI and the ESTOI value from the same LDS block
//   st_finish_kernel / mr_finish_kernel / sd_finish_kernel   one workgroup per utterance sums its partials in index order
//   sd_partial_kernel      the five sums of SI-SDR per tile of 4096 samples
// No floating-point atomics, no workgroup waits on another; every sum is taken in an order fixed by the utterance's own indices, so a
// row's result depends on nothing but the row.  Nothing at or beyond lens[b] is read.
#include "ctts_common.h"
#include "fft_common.h"
#include <math.h>
#include <algorithm>

namespace {

constexpr int WM_THREADS = 256;
constexpr int ST_FRAME = 256, ST_HOP = 128, ST_NFFT = 512, ST_BANDS = 15, ST_SEG = 30;
constexpr int ST_MAX_FRAMES = 8192;              // frames per utterance: 81.9 s at 10 kHz
constexpr double ST_EPS = 2.220446049250313e-16; // 2^-52
constexpr double ST_RANGE_DB = 40.0;
constexpr int SD_TILE = 4096;
constexpr double MR_CLAMP = 1e-7;
enum { EPI_STOI = 0, EPI_MR = 1 };

// band j covers the bins [ST_EDGE[j], ST_EDGE[j + 1]): nearest bins to 150 * 2^((2j -+ 1) / 6) Hz on the 10000 / 512 Hz grid
__constant__ int ST_EDGE[ST_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

__host__ __device__ __forceinline__ int wm_frames(int len, int win, int hop) { return len >= win ? (len - win) / hop + 1 : 0; }

// ---------------------------------------------------------------- STOI: silent-frame step
__global__ __launch_bounds__(WM_THREADS) void st_energy_kernel(const float* __restrict__ ref, const int32_t* __restrict__ lens,
                                                               const double* __restrict__ w, double* __restrict__ energy, int N, int Fa) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int len = min(max(lens[b], 0), N);
  if (i >= min(wm_frames(len, ST_FRAME, ST_HOP), Fa)) return;       // wave-uniform; no barrier below
  const float* x = ref + (long)b * N + (long)i * ST_HOP;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double p = w[lane + 64 * q] * (double)x[lane + 64 * q];
    s = fma(p, p, s);
  }
  s = ctts_wave_sum_d(s);
  if (lane == 0) energy[(long)b * Fa + i] = s;
}

__device__ __forceinline__ double st_db(double s) { return 20.0 * log10(sqrt(s) + ST_EPS); }

__global__ __launch_bounds__(WM_THREADS) void st_keep_kernel(const double* __restrict__ energy, const int32_t* __restrict__ lens,
                                                             int32_t* __restrict__ idx, int32_t* __restrict__ counts, int N, int Fa) {
  __shared__ double smax[WM_THREADS];
  __shared__ int scnt[WM_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const int F = min(wm_frames(len, ST_FRAME, ST_HOP), Fa);
  const double* e = energy + (long)b * Fa;
  double m = 0.0;
  for (int i = tid; i < F; i += WM_THREADS) m = fmax(m, e[i]);
  smax[tid] = m;
  __syncthreads();
  for (int h = WM_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) smax[tid] = fmax(smax[tid], smax[tid + h]);
    __syncthreads();
  }
  m = smax[0];
  const double thr = st_db(m) - ST_RANGE_DB;
  const int per = (F + WM_THREADS - 1) / WM_THREADS;
  const int i0 = min(tid * per, F), i1 = min(i0 + per, F);
  int c = 0;
  for (int i = i0; i < i1; ++i) c += st_db(e[i]) > thr ? 1 : 0;
  scnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < WM_THREADS; ++t) {
      const int v = scnt[t];
      scnt[t] = run;
      run += v;
    }
    counts[b * 3 + 0] = F;
    counts[b * 3 + 1] = run;
    counts[b * 3 + 2] = (m > 0.0 && run >= ST_SEG) ? run - (ST_SEG - 1) : 0;
  }
  __syncthreads();
  int o = scnt[tid];
  int32_t* ix = idx + (long)b * Fa;
  for (int i = i0; i < i1; ++i)
    if (st_db(e[i]) > thr) ix[o++] = i;                             // o < kept <= F <= Fa
}

// ---------------------------------------------------------------- the shared frame-spectrum kernel
// EPI_STOI: idx / counts drive the gather and `out` receives the band amplitudes [B][2][15][Fa];  EPI_MR: plain framing at fr * hop (idx and
// counts are NULL) and `out` receives the frame partials [B][Fa][4].  Fa is the frame stride of the workspace rows.
template <int NFFT, int EPI>
__global__ __launch_bounds__(WM_THREADS) void frame_spectrum(const float* __restrict__ ref, const float* __restrict__ syn,
                                                             const int32_t* __restrict__ lens, const double* __restrict__ w,
                                                             const int32_t* __restrict__ idx, const int32_t* __restrict__ counts,
                                                             double* __restrict__ out, int N, int Fa, int hop, int win) {
  __shared__ double2 a[NFFT];
  __shared__ double2 tw[NFFT / 2];
  __shared__ double red[EPI == EPI_MR ? 4 * WM_THREADS : 1];
  const int b = blockIdx.y, fr = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const float* x = ref + (long)b * N;
  const float* y = syn + (long)b * N;
  int kept = 0;
  if (EPI == EPI_STOI) {
    kept = min(counts[b * 3 + 1], Fa);
    if (fr >= kept) return;                                         // workgroup-uniform
  } else {
    if (fr >= wm_frames(len, win, hop)) return;
  }
  ctts_dfft_fill_twiddles<NFFT, WM_THREADS>(tw, tid);
  for (int n = tid; n < NFFT; n += WM_THREADS) {
    double vx = 0.0, vy = 0.0;
    if (EPI == EPI_STOI) {
      if (n < ST_FRAME) {
        // sample n of frame fr of the compacted signal: the kept frames, windowed, overlap-added at hop 128 in kept order
        const int32_t* ix = idx + (long)b * Fa;
        const long p0 = (long)ix[fr] * ST_HOP + n;                  // a kept frame lies inside [0, len)
        vx = w[n] * (double)x[p0];
        vy = w[n] * (double)y[p0];
        if (n < ST_HOP && fr > 0) {
          const long p1 = (long)ix[fr - 1] * ST_HOP + n + ST_HOP;
          vx += w[n + ST_HOP] * (double)x[p1];
          vy += w[n + ST_HOP] * (double)y[p1];
        } else if (n >= ST_HOP && fr + 1 < kept) {
          const long p1 = (long)ix[fr + 1] * ST_HOP + n - ST_HOP;
          vx += w[n - ST_HOP] * (double)x[p1];
          vy += w[n - ST_HOP] * (double)y[p1];
        }
        vx *= w[n];
        vy *= w[n];
      }
    } else if (n < win) {
      const long p0 = (long)fr * hop + n;                           // < len: fr < frames(len)
      vx = w[n] * (double)x[p0];
      vy = w[n] * (double)y[p0];
    }
    a[ctts_dfft_slot<NFFT>(n)] = make_double2(vx, vy);
  }
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < ctts_log2<NFFT>::value; ++s) ctts_dfft_pass<NFFT, WM_THREADS>(a, tw, s, tid);
  // Z = X + i Y with X, Y Hermitian:  |X_k|^2 = ((a + c)^2 + (b - d)^2) / 4,  |Y_k|^2 = ((b + d)^2 + (a - c)^2) / 4,  Z_k = a + i b, Z_{N-k} = c + i d
  auto power = [&](int k, double& px, double& py) {
    const double2 zk = a[k], zn = a[(NFFT - k) & (NFFT - 1)];
    const double xr = zk.x + zn.x, xi = zk.y - zn.y, yr = zk.y + zn.y, yi = zk.x - zn.x;
    px = 0.25 * (xr * xr + xi * xi);
    py = 0.25 * (yr * yr + yi * yi);
  };
  if (EPI == EPI_STOI) {
    if (tid < 2 * ST_BANDS) {
      const int sig = tid / ST_BANDS, j = tid % ST_BANDS;
      double s = 0.0;
      for (int k = ST_EDGE[j]; k < ST_EDGE[j + 1]; ++k) {
        double px, py;
        power(k, px, py);
        s += sig ? py : px;
      }
      out[(((long)b * 2 + sig) * ST_BANDS + j) * Fa + fr] = sqrt(s);
    }
  } else {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = tid; k <= NFFT / 2; k += WM_THREADS) {
      double px, py;
      power(k, px, py);
      px = fmax(px, MR_CLAMP);
      py = fmax(py, MR_CLAMP);
      const double d = sqrt(px) - sqrt(py), l = 0.5 * (log(px) - log(py));
      v[0] = fma(d, d, v[0]);
      v[1] += px;
      v[2] += fabs(l);
      v[3] = fma(l, l, v[3]);
    }
    ctts_block_tree_sum<4, WM_THREADS>(v, red);
    if (tid == 0) {
      double* p = out + ((long)b * Fa + fr) * 4;
      p[0] = v[0];
      p[1] = v[1];
      p[2] = v[2];
      p[3] = (20.0 / 2.302585092994046) * sqrt(v[3] / (double)(NFFT / 2 + 1));
    }
  }
}

__global__ __launch_bounds__(WM_THREADS) void mr_finish_kernel(const double* __restrict__ part, const int32_t* __restrict__ lens,
                                                               double* __restrict__ out, int32_t* __restrict__ frames, int N, int Fa, int hop,
                                                               int win, int nbins) {
  __shared__ double red[4 * WM_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const int nf = min(wm_frames(len, win, hop), Fa);
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < nf; i += WM_THREADS) {
    const double* p = part + ((long)b * Fa + i) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += p[k];
  }
  ctts_block_tree_sum<4, WM_THREADS>(v, red);
  if (tid == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    out[b * 3 + 0] = nf > 0 ? sqrt(v[0] / v[1]) : nan;
    out[b * 3 + 1] = nf > 0 ? v[2] / ((double)nf * (double)nbins) : nan;
    out[b * 3 + 2] = nf > 0 ? v[3] / (double)nf : nan;
    frames[b] = nf;
  }
}

// ---------------------------------------------------------------- STOI: segments
__global__ __launch_bounds__(64) void st_segment_kernel(const double* __restrict__ bands, const int32_t* __restrict__ counts,
                                                        double* __restrict__ segv, int Fa) {
  constexpr int LD = ST_SEG + 1;
  __shared__ double X[ST_BANDS * LD], Y[ST_BANDS * LD], Xn[ST_BANDS * LD], Yn[ST_BANDS * LD];
  __shared__ double dj[ST_BANDS], col[ST_SEG];
  const int b = blockIdx.y, s = blockIdx.x, lane = threadIdx.x;
  if (s >= min(counts[b * 3 + 2], Fa - (ST_SEG - 1))) return;       // workgroup-uniform
  for (int e = lane; e < 2 * ST_BANDS * ST_SEG; e += 64) {
    const int sig = e / (ST_BANDS * ST_SEG), r = e % (ST_BANDS * ST_SEG), j = r / ST_SEG, n = r % ST_SEG;
    const double v = bands[(((long)b * 2 + sig) * ST_BANDS + j) * Fa + s + n];      // s + n < kept <= Fa
    (sig ? Y : X)[j * LD + n] = v;
  }
  __syncthreads();
  if (lane < ST_BANDS) {                                            // STOI: one band row per lane
    const double* xr = X + lane * LD;
    const double* yr = Y + lane * LD;
    double sx = 0.0, sy = 0.0;
    for (int n = 0; n < ST_SEG; ++n) {
      sx = fma(xr[n], xr[n], sx);
      sy = fma(yr[n], yr[n], sy);
    }
    const double alpha = sqrt(sx) / (sqrt(sy) + ST_EPS);
    const double clip = 1.0 + 5.623413251903491;                    // 1 + 10^(15 / 20)
    double mx = 0.0, my = 0.0;
    for (int n = 0; n < ST_SEG; ++n) {
      mx += xr[n];
      my += fmin(alpha * yr[n], xr[n] * clip);
    }
    mx /= (double)ST_SEG;
    my /= (double)ST_SEG;
    double cxx = 0.0, cyy = 0.0, cxy = 0.0;
    for (int n = 0; n < ST_SEG; ++n) {
      const double xc = xr[n] - mx, yc = fmin(alpha * yr[n], xr[n] * clip) - my;
      cxx = fma(xc, xc, cxx);
      cyy = fma(yc, yc, cyy);
      cxy = fma(xc, yc, cxy);
    }
    dj[lane] = cxy / ((sqrt(cxx) + ST_EPS) * (sqrt(cyy) + ST_EPS));
  }
  if (lane < 2 * ST_BANDS) {                                        // ESTOI: rows mean-removed and normalised
    const int sig = lane / ST_BANDS, j = lane % ST_BANDS;
    const double* r = (sig ? Y : X) + j * LD;
    double* o = (sig ? Yn : Xn) + j * LD;
    double m = 0.0, q = 0.0;
    for (int n = 0; n < ST_SEG; ++n) m += r[n];
    m /= (double)ST_SEG;
    for (int n = 0; n < ST_SEG; ++n) q = fma(r[n] - m, r[n] - m, q);
    const double inv = sqrt(q) + ST_EPS;
    for (int n = 0; n < ST_SEG; ++n) o[n] = (r[n] - m) / inv;
  }
  __syncthreads();
  if (lane < 2 * ST_SEG) {                                          // then columns
    const int sig = lane / ST_SEG, n = lane % ST_SEG;
    double* c = (sig ? Yn : Xn) + n;
    double m = 0.0, q = 0.0;
    for (int j = 0; j < ST_BANDS; ++j) m += c[j * LD];
    m /= (double)ST_BANDS;
    for (int j = 0; j < ST_BANDS; ++j) q = fma(c[j * LD] - m, c[j * LD] - m, q);
    const double inv = sqrt(q) + ST_EPS;
    for (int j = 0; j < ST_BANDS; ++j) c[j * LD] = (c[j * LD] - m) / inv;
  }
  __syncthreads();
  if (lane < ST_SEG) {
    double t = 0.0;
    for (int j = 0; j < ST_BANDS; ++j) t = fma(Xn[j * LD + lane], Yn[j * LD + lane], t);
    col[lane] = t;
  }
  __syncthreads();
  if (lane == 0) {
    double d = 0.0, e = 0.0;
    for (int j = 0; j < ST_BANDS; ++j) d += dj[j];
    for (int n = 0; n < ST_SEG; ++n) e += col[n];
    segv[((long)b * Fa + s) * 2 + 0] = d;
    segv[((long)b * Fa + s) * 2 + 1] = e / (double)ST_SEG;
  }
}

__global__ __launch_bounds__(WM_THREADS) void st_finish_kernel(const double* __restrict__ segv, const int32_t* __restrict__ counts,
                                                               double* __restrict__ stoi, double* __restrict__ estoi, int Fa) {
  __shared__ double red[2 * WM_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int S = min(counts[b * 3 + 2], max(Fa - (ST_SEG - 1), 0));
  double v[2] = {0.0, 0.0};
  for (int s = tid; s < S; s += WM_THREADS) {
    v[0] += segv[((long)b * Fa + s) * 2 + 0];
    v[1] += segv[((long)b * Fa + s) * 2 + 1];
  }
  ctts_block_tree_sum<2, WM_THREADS>(v, red);
  if (tid == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    stoi[b] = S > 0 ? v[0] / ((double)ST_BANDS * (double)S) : nan;
    estoi[b] = S > 0 ? v[1] / (double)S : nan;
  }
}

// frames / kept / segments of utterances too short for one frame, when no row of the batch holds 256 samples
__global__ void st_empty_kernel(double* __restrict__ stoi, double* __restrict__ estoi, int32_t* __restrict__ counts, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  stoi[b] = nan;
  estoi[b] = nan;
  counts[b * 3 + 0] = counts[b * 3 + 1] = counts[b * 3 + 2] = 0;
}

// ---------------------------------------------------------------- SI-SDR
__global__ __launch_bounds__(WM_THREADS) void sd_partial_kernel(const float* __restrict__ ref, const float* __restrict__ syn,
                                                                const int32_t* __restrict__ lens, double* __restrict__ part, int N, int nt) {
  __shared__ double red[5 * WM_THREADS];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const int t0 = tile * SD_TILE;
  if (t0 >= len) return;                                            // workgroup-uniform
  const float* x = ref + (long)b * N;
  const float* y = syn + (long)b * N;
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int q = 0; q < SD_TILE / WM_THREADS; ++q) {
    const int i = t0 + q * WM_THREADS + tid;
    if (i < len) {
      const double xd = (double)x[i], yd = (double)y[i];
      v[0] += xd;
      v[1] += yd;
      v[2] = fma(xd, yd, v[2]);
      v[3] = fma(xd, xd, v[3]);
      v[4] = fma(yd, yd, v[4]);
    }
  }
  ctts_block_tree_sum<5, WM_THREADS>(v, red);
  if (tid == 0) {
    double* p = part + ((long)b * nt + tile) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) p[k] = v[k];
  }
}

__global__ __launch_bounds__(WM_THREADS) void sd_finish_kernel(const double* __restrict__ part, const int32_t* __restrict__ lens,
                                                               double* __restrict__ out, int N, int nt) {
  __shared__ double red[5 * WM_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), N);
  const int ntl = min((len + SD_TILE - 1) / SD_TILE, nt);
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = tid; t < ntl; t += WM_THREADS) {
    const double* p = part + ((long)b * nt + t) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] += p[k];
  }
  ctts_block_tree_sum<5, WM_THREADS>(v, red);
  if (tid == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double r = nan;
    if (len > 0) {
      const double n = (double)len;
      const double cxx = v[3] - v[0] * v[0] / n, cxy = v[2] - v[0] * v[1] / n, cyy = v[4] - v[1] * v[1] / n;
      if (cxx > 0.0) {
        const double alpha = cxy / cxx;
        const double tgt = alpha * alpha * cxx;                     // ||t||^2
        const double noise = (cyy - 2.0 * alpha * cxy) + tgt;       // ||y - t||^2: exactly 0 for y = 2^k x
        if (noise > 0.0) r = 10.0 * log10(tgt / noise);
        else if (tgt > 0.0) r = INFINITY;
      }
    }
    out[b] = r;
  }
}

size_t st_frames_alloc(int N) { return (size_t)std::max(wm_frames(N, ST_FRAME, ST_HOP), 1); }

}  // namespace

extern "C" int ctts_stoi_max_frames(void) { return ST_MAX_FRAMES; }

extern "C" size_t ctts_stoi_workspace_bytes(int B, int N) {
  if (B < 1 || N < 1 || wm_frames(N, ST_FRAME, ST_HOP) > ST_MAX_FRAMES) return 0;
  const size_t Fa = st_frames_alloc(N);
  // energy [B][Fa], bands [B][2][15][Fa], segv [B][Fa][2] (double), idx [B][Fa] (int32, padded to 8 bytes)
  return sizeof(double) * (size_t)B * Fa * (1 + 2 * ST_BANDS + 2) + sizeof(double) * (((size_t)B * Fa + 1) / 2);
}

extern "C" int ctts_stoi(const float* ref, const float* syn, const int32_t* lens, const double* window, double* stoi, double* estoi,
                         int32_t* counts, int B, int N, void* workspace, void* stream) {
  CTTS_REQUIRE(ref && syn && lens && window && stoi && estoi && counts && workspace && B > 0 && N > 0, "ctts_stoi: bad arguments");
  CTTS_REQUIRE(B <= 65535, "ctts_stoi: at most 65535 utterances per call (got %d)", B);
  const int Fm = wm_frames(N, ST_FRAME, ST_HOP);
  CTTS_REQUIRE(Fm <= ST_MAX_FRAMES, "ctts_stoi: rows of %d samples hold %d frames; at most %d (%d samples) per utterance", N, Fm, ST_MAX_FRAMES,
               ST_HOP * (ST_MAX_FRAMES - 1) + ST_FRAME);
  hipStream_t st = (hipStream_t)stream;
  if (Fm == 0) {
    hipLaunchKernelGGL(st_empty_kernel, dim3((B + 63) / 64), dim3(64), 0, st, stoi, estoi, counts, B);
    CTTS_CHECK_LAUNCH("ctts_stoi (no frame)");
    return 0;
  }
  const int Fa = Fm;
  double* energy = (double*)workspace;
  double* bands = energy + (size_t)B * Fa;
  double* segv = bands + (size_t)B * Fa * 2 * ST_BANDS;
  int32_t* idx = (int32_t*)(segv + (size_t)B * Fa * 2);
  hipLaunchKernelGGL(st_energy_kernel, dim3((Fm + 3) / 4, B), dim3(WM_THREADS), 0, st, ref, lens, window, energy, N, Fa);
  CTTS_CHECK_LAUNCH("ctts_stoi (frame energies)");
  hipLaunchKernelGGL(st_keep_kernel, dim3(B), dim3(WM_THREADS), 0, st, energy, lens, idx, counts, N, Fa);
  CTTS_CHECK_LAUNCH("ctts_stoi (silent-frame removal)");
  hipLaunchKernelGGL((frame_spectrum<ST_NFFT, EPI_STOI>), dim3(Fm, B), dim3(WM_THREADS), 0, st, ref, syn, lens, window, idx, counts, bands, N, Fa,
                     ST_HOP, ST_FRAME);
  CTTS_CHECK_LAUNCH("ctts_stoi (band amplitudes)");
  if (Fm >= ST_SEG) {
    hipLaunchKernelGGL(st_segment_kernel, dim3(Fm - (ST_SEG - 1), B), dim3(64), 0, st, bands, counts, segv, Fa);
    CTTS_CHECK_LAUNCH("ctts_stoi (segments)");
  }
  hipLaunchKernelGGL(st_finish_kernel, dim3(B), dim3(WM_THREADS), 0, st, segv, counts, stoi, estoi, Fa);
  CTTS_CHECK_LAUNCH("ctts_stoi");
  return 0;
}

extern "C" size_t ctts_si_sdr_workspace_bytes(int B, int N) {
  if (B < 1 || N < 1) return 0;
  return sizeof(double) * 5 * (size_t)B * (size_t)((N + SD_TILE - 1) / SD_TILE);
}

extern "C" int ctts_si_sdr(const float* ref, const float* syn, const int32_t* lens, double* out, int B, int N, void* workspace, void* stream) {
  CTTS_REQUIRE(ref && syn && lens && out && workspace && B > 0 && N > 0, "ctts_si_sdr: bad arguments");
  CTTS_REQUIRE(B <= 65535 && N <= (1 << 30), "ctts_si_sdr: at most 65535 utterances of 2^30 samples (got %d x %d)", B, N);
  hipStream_t st = (hipStream_t)stream;
  const int nt = (N + SD_TILE - 1) / SD_TILE;
  hipLaunchKernelGGL(sd_partial_kernel, dim3(nt, B), dim3(WM_THREADS), 0, st, ref, syn, lens, (double*)workspace, N, nt);
  CTTS_CHECK_LAUNCH("ctts_si_sdr (tile sums)");
  hipLaunchKernelGGL(sd_finish_kernel, dim3(B), dim3(WM_THREADS), 0, st, (const double*)workspace, lens, out, N, nt);
  CTTS_CHECK_LAUNCH("ctts_si_sdr");
  return 0;
}

extern "C" size_t ctts_mr_stft_workspace_bytes(int B, int N, int hop, int win) {
  if (B < 1 || N < 1 || hop < 1 || win < 1 || N > (1 << 30)) return 0;
  return sizeof(double) * 4 * (size_t)B * (size_t)std::max(wm_frames(N, win, hop), 1);
}

extern "C" int ctts_mr_stft(const float* ref, const float* syn, const int32_t* lens, const double* window, double* out, int32_t* frames, int B,
                            int N, int n_fft, int hop, int win, void* workspace, void* stream) {
  CTTS_REQUIRE(ref && syn && lens && window && out && frames && workspace && B > 0 && N > 0, "ctts_mr_stft: bad arguments");
  CTTS_REQUIRE(B <= 65535 && N <= (1 << 30), "ctts_mr_stft: at most 65535 utterances of 2^30 samples (got %d x %d)", B, N);
  CTTS_REQUIRE(n_fft == 512 || n_fft == 1024 || n_fft == 2048, "ctts_mr_stft: n_fft must be 512, 1024 or 2048 (got %d)", n_fft);
  CTTS_REQUIRE(win >= 1 && win <= n_fft && hop >= 1, "ctts_mr_stft: need 1 <= win <= n_fft and hop >= 1 (got win %d, hop %d, n_fft %d)", win, hop,
               n_fft);
  hipStream_t st = (hipStream_t)stream;
  const int Fm = wm_frames(N, win, hop), Fa = std::max(Fm, 1);
  double* part = (double*)workspace;
  if (Fm > 0) {
    const dim3 grid(Fm, B);
    if (n_fft == 512)
      hipLaunchKernelGGL((frame_spectrum<512, EPI_MR>), grid, dim3(WM_THREADS), 0, st, ref, syn, lens, window, nullptr, nullptr, part, N, Fa, hop, win);
    else if (n_fft == 1024)
      hipLaunchKernelGGL((frame_spectrum<1024, EPI_MR>), grid, dim3(WM_THREADS), 0, st, ref, syn, lens, window, nullptr, nullptr, part, N, Fa, hop, win);
    else
      hipLaunchKernelGGL((frame_spectrum<2048, EPI_MR>), grid, dim3(WM_THREADS), 0, st, ref, syn, lens, window, nullptr, nullptr, part, N, Fa, hop, win);
    CTTS_CHECK_LAUNCH("ctts_mr_stft (frame spectra)");
  }
  hipLaunchKernelGGL(mr_finish_kernel, dim3(B), dim3(WM_THREADS), 0, st, part, lens, out, frames, N, Fa, hop, win, n_fft / 2 + 1);
  CTTS_CHECK_LAUNCH("ctts_mr_stft");
  return 0;
}
