// HiFi-GAN V1 generator (reference hifigan/models.py:112-173) inference kernels: every Conv1d of the network as ONE launch.
//
// vconv_kernel: dilated Conv1d (stride 1, zero padding d (k - 1) / 2) and ConvTranspose1d as an implicit GEMM on the MFMA.
//   rows = (b, position p), N = output columns, K = taps x Cin.  A workgroup owns 128 positions of one utterance x BN columns.  For every
//   32-channel chunk of the input it stages its 128 rows PLUS the (taps - 1) x dil halo into LDS once (on-load leaky_relu, zero rows
//   outside [0, T)); every tap then reads a row-shifted view of that tile, so an input element is fetched and split once per tile and
//   chunk, not once per tap.  The weights arrive pre-packed [roundup(N, 128)][taps][roundup(Cin, 32)] (and, for the split arithmetic,
//   pre-split by ctts_split_planes: they are constant) and one tap's 32-deep K-block is staged per step, prefetched into registers
//   while the previous one is multiplied.
//   ConvTranspose1d(stride u, kernel K, pad (K - u) / 2) is the polyphase form: output t = q u + r - pad = sum_j x[q - j] W[:, :, r + j u]
//   (j < K / u) is a K/u-tap stride-1 conv over INPUT time whose N = u x Cout columns hold all phases (column r Cout + co); the epilogue
//   scatters row q's phases to output rows q u + r - pad and drops those outside [0, T u).
//   Epilogue: out = beta * out + alpha * (acc + bias + R) (beta == 0 never reads out): the ResBlock's `x = xt + x` (models.py:103), the
//   generator's `xs += resblock(x)` and `/ num_kernels` (models.py:153-160) without elementwise passes.
//   Arithmetic (include/ctts.h ctts_vocoder_conv): X6 = the exact three-way bf16 split (planes_common.h spl_one) with the six cross terms on
//   v_mfma_f32_32x32x16_bf16, fp32 accumulation; otherwise exact fp32 on v_mfma_f32_32x32x2_f32.  No atomics: every output element is
//   produced by one lane in a fixed order.
//   Length-aware batches (include/ctts.h, lens / len_mul): a workgroup reads lens[b] once (wave-uniform) and its utterance's own row
//   count Tb = min(lens[b] len_mul, T) takes T's place in the staging, the halo, the epilogue's row bound (R and beta * out included)
//   and the transposed conv's row range and phase scatter; a tile at or beyond its utterance's end returns before it stages anything.
//   The grid is still sized by the padded T and anchored at row 0 of each utterance, so a tile computes bit for bit what the same tile
//   of a B = 1 call on the unpadded utterance computes.  Rows beyond Tb are not stored (nothing reads them).
// vpost_kernel: conv_post (Cout = 1, models.py:161-163) - leaky_relu(0.01) on load, 7-tap dot product on the VALU, + bias, tanh;
//   with lens it writes exact zeros from row Tb on (whole tiles beyond the end without staging).
#include "ctts_common.h"
#include "planes_common.h"

namespace {

typedef float vc_floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 vc_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int vc_u32x4 __attribute__((ext_vector_type(4)));

constexpr int VC_BM = 128;                 // positions per workgroup
constexpr int VC_HALO_MAX = 64;            // (taps - 1) x dil: V1's largest is (11 - 1) x 5 = 50
constexpr int VC_AROWS = VC_BM + VC_HALO_MAX;
// X6 LDS: per operand three planes (hi | mid | lo) of 64-byte rows = 32 bf16 of one chunk; 16-byte chunks XOR-swizzled by (row >> 2) & 3
constexpr int VC_X6_APLANE = VC_AROWS * 64, VC_X6_BPLANE = 128 * 64;
// fp32 LDS: 128-byte rows = 32 floats; 16-byte chunks XOR-swizzled by (row >> 1) & 7
constexpr int VC_F32_A = VC_AROWS * 128, VC_F32_B = 128 * 128;
constexpr int VC_LDS_X6 = 3 * VC_X6_APLANE + 3 * VC_X6_BPLANE;     // 61,440 bytes
constexpr int VC_LDS_F32 = VC_F32_A + VC_F32_B;                     // 40,960 bytes

struct VcParams {
  const float* x; long sxb, sxt, sxc;
  int T, Cin, cin_pad, taps, dil, in_off, row_off, Mrows, N, Cout, u, pad, Tout;
  int act_in; float slope; int vec;
  const float* w; const uint16_t* wp; const float* bias; const float* R; float* out;
  float alpha, beta;
  const int* lens; int len_mul, mextra;     // ragged: utterance b's input has min(lens[b] len_mul, T) rows; Mrows = T + mextra
};

// rows of utterance b's signal at a layer whose dense length is T: min(max(lens[b], 0) len_mul, T); lens == NULL: T (wave-uniform)
__device__ __forceinline__ int vc_rows(const int* lens, int b, int len_mul, int T) {
  if (!lens) return T;
  const long n = (long)max(lens[b], 0) * len_mul;
  return n < (long)T ? (int)n : T;
}

__device__ __forceinline__ int x6sw(int row, int c) { return c ^ ((row >> 2) & 3); }
__device__ __forceinline__ int f32sw(int row, int c) { return c ^ ((row >> 1) & 7); }

template <bool X6, int BN>
__global__ __launch_bounds__(256, 2) void vconv_kernel(const VcParams p) {
  constexpr int NT = BN == 128 ? 2 : 1;
  constexpr int WAVES_N = BN / (32 * NT);             // 2, 2, 1
  constexpr int WAVES_M = 4 / WAVES_N;                // 2, 2, 4
  constexpr int MT = VC_BM / (32 * WAVES_M);          // 2, 2, 1
  constexpr int B_CHUNKS = X6 ? BN * 12 : BN * 8;     // 16-byte pieces of one staged weight K-block
  constexpr int B_PER_T = (B_CHUNKS + 255) / 256;
  __shared__ __attribute__((aligned(16))) unsigned char smem[X6 ? VC_LDS_X6 : VC_LDS_F32];
  unsigned char* sA = smem;
  unsigned char* sB = smem + (X6 ? 3 * VC_X6_APLANE : VC_F32_A);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, m0 = blockIdx.x * VC_BM, col0 = blockIdx.y * BN;
  const int wm0 = (wave / WAVES_N) * (MT * 32), wn0 = (wave % WAVES_N) * (NT * 32);
  // ragged (include/ctts.h): the utterance's own length replaces T everywhere below; a tile at or beyond its end has nothing to do
  const int Tb = vc_rows(p.lens, b, p.len_mul, p.T), Mb = Tb + p.mextra, Toutb = p.u ? Tb * p.u : Tb;
  if (Tb == 0 || m0 >= Mb) return;
  const int p0 = p.row_off + m0;                      // position of tile row 0
  const int nchunks = p.cin_pad >> 5, taps = p.taps;
  const long kp = (long)taps * p.cin_pad;             // packed weight row length
  const int arows = VC_BM + (taps - 1) * p.dil;
  const float* xb = p.x + (long)b * p.sxb;

  vc_floatx16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  vc_u32x4 rb[B_PER_T];
  // weight K-block kbg (= tap * nchunks + chunk) of columns col0 .. col0 + BN into registers (the packed rows are padded to 128 columns)
  auto load_b = [&](int kbg) {
#pragma unroll
    for (int i = 0; i < B_PER_T; ++i) {
      const int idx = tid + 256 * i;
      if (B_CHUNKS % 256 == 0 || idx < B_CHUNKS) {
        if constexpr (X6) {
          const int n = idx / 12, part = idx - n * 12;
          rb[i] = *reinterpret_cast<const vc_u32x4*>(p.wp + ((long)(col0 + n) * kp + (long)kbg * 32) * 3 + part * 8);
        } else {
          const int n = idx >> 3, c = idx & 7;
          rb[i] = *reinterpret_cast<const vc_u32x4*>(p.w + (long)(col0 + n) * kp + (long)kbg * 32 + c * 4);
        }
      }
    }
  };
  auto store_b = [&]() {
#pragma unroll
    for (int i = 0; i < B_PER_T; ++i) {
      const int idx = tid + 256 * i;
      if (B_CHUNKS % 256 == 0 || idx < B_CHUNKS) {
        if constexpr (X6) {
          const int n = idx / 12, part = idx - n * 12, q = part >> 2, c = part & 3;
          *reinterpret_cast<vc_u32x4*>(sB + q * VC_X6_BPLANE + n * 64 + x6sw(n, c) * 16) = rb[i];
        } else {
          const int n = idx >> 3, c = idx & 7;
          *reinterpret_cast<vc_u32x4*>(sB + n * 128 + f32sw(n, c) * 16) = rb[i];
        }
      }
    }
  };
  // input rows p0 + in_off + i (i < arows), channels chunk * 32 .. + 31, activated, zero outside [0, T) x [0, Cin)   (T = the utterance's Tb)
  auto stage_a = [&](int chunk) {
    const int c4 = tid & 7, cbase = chunk * 32 + c4 * 4;
    for (int i = tid >> 3; i < arows; i += 32) {
      const int ti = p0 + p.in_off + i;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (ti >= 0 && ti < Tb) {
        const float* src = xb + (long)ti * p.sxt;
        if (p.vec) {
          if (cbase < p.Cin) {
            const float4 f = *reinterpret_cast<const float4*>(src + cbase);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (cbase + e < p.Cin) v[e] = src[(long)(cbase + e) * p.sxc];
        }
        if (p.act_in) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * p.slope;
        }
      }
      if constexpr (X6) {
        unsigned hi[4], mid[4], lo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) spl_one(v[e], hi[e], mid[e], lo[e]);
        unsigned char* o = sA + i * 64 + x6sw(i, c4 >> 1) * 16 + (c4 & 1) * 8;
        *reinterpret_cast<uint2*>(o) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
        *reinterpret_cast<uint2*>(o + VC_X6_APLANE) = make_uint2(mid[0] | (mid[1] << 16), mid[2] | (mid[3] << 16));
        *reinterpret_cast<uint2*>(o + 2 * VC_X6_APLANE) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
      } else {
        *reinterpret_cast<float4*>(sA + i * 128 + f32sw(i, c4) * 16) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  };
  auto compute = [&](int shift) {
    if constexpr (X6) {
      vc_u32x4 fa[2][MT][3], fb[2][NT][3];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const int row = wm0 + i * 32 + l31 + shift;
#pragma unroll
          for (int q = 0; q < 3; ++q)
            fa[ks][i][q] = *reinterpret_cast<const vc_u32x4*>(sA + q * VC_X6_APLANE + row * 64 + x6sw(row, ks * 2 + h) * 16);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int row = wn0 + j * 32 + l31;
#pragma unroll
          for (int q = 0; q < 3; ++q)
            fb[ks][j][q] = *reinterpret_cast<const vc_u32x4*>(sB + q * VC_X6_BPLANE + row * 64 + x6sw(row, ks * 2 + h) * 16);
        }
      }
      // six cross terms, smallest first, consecutive MFMAs on different accumulators (the order of gemm.hip's x6 kernel)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < 6; ++t) {
          constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(vc_bf16x8, fa[ks][i][PA[t]]),
                                                                  __builtin_bit_cast(vc_bf16x8, fb[ks][j][PB[t]]), acc[i][j], 0, 0, 0);
        }
    } else {
      // lane (l31, h) supplies k = 16 h + s to MFMA step s (a fixed permutation of the 32-deep block, the same for A and B)
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        float4 fa[MT], fb[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const int row = wm0 + i * 32 + l31 + shift;
          fa[i] = *reinterpret_cast<const float4*>(sA + row * 128 + f32sw(row, h * 4 + s4) * 16);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int row = wn0 + j * 32 + l31;
          fb[j] = *reinterpret_cast<const float4*>(sB + row * 128 + f32sw(row, h * 4 + s4) * 16);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
      }
    }
  };

  load_b(0);
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    __syncthreads();                       // every wave is done with the previous chunk's tiles
    stage_a(chunk);
    store_b();
    __syncthreads();
    for (int tap = 0; tap < taps; ++tap) {
      int nt = tap + 1, nc = chunk;
      if (nt == taps) { nt = 0; ++nc; }
      if (nc == nchunks) { nt = tap; nc = chunk; }     // the last block is fetched again: keeps the staging registers in registers
      load_b(nt * nchunks + nc);
      compute(tap * p.dil);
      if (tap + 1 < taps) {
        __syncthreads();
        store_b();
        __syncthreads();
      }
    }
  }

  // epilogue: element (row wm0 + 32 i + (r & 3) + 8 (r >> 2) + 4 h, column wn0 + 32 j + l31) of the wave's tiles
  const long obase = (long)b * p.Tout * p.Cout;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = col0 + wn0 + j * 32 + l31;
    if (n >= p.N) continue;
    int ph = 0, co = n;
    if (p.u) { ph = n / p.Cout; co = n - ph * p.Cout; }
    const float bv = p.bias ? p.bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ml = wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m0 + ml >= Mb) continue;
        const int pos = p0 + ml;
        const int to = p.u ? pos * p.u + ph - p.pad : pos;
        if (to < 0 || to >= Toutb) continue;
        const long idx = obase + (long)to * p.Cout + co;
        float v = acc[i][j][r] + bv;
        if (p.R) v += p.R[idx];
        v *= p.alpha;
        if (p.beta != 0.f) v = p.beta * p.out[idx] + v;
        p.out[idx] = v;
      }
  }
}

constexpr int VP_ROWS = 256, VP_PITCH = 33;

// out[b, 0, t] = tanh(bias + sum_{tap, c} leaky_relu(x[b, t + tap - (k - 1) / 2, c], slope) w[tap][c]); x [B, T, C] dense
// ragged (lens != NULL): rows at or beyond Tb = min(lens[b] len_mul, T) read as zero and out[b, 0, Tb ..] = 0
__global__ __launch_bounds__(256) void vpost_kernel(const float* __restrict__ x, int T, int C, int k, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float slope, float* __restrict__ out,
                                                    const int* __restrict__ lens, int len_mul) {
  extern __shared__ float xs[];
  const int b = blockIdx.y, t0 = blockIdx.x * VP_ROWS, tid = threadIdx.x, half = (k - 1) / 2;
  const int rows = VP_ROWS + k - 1;
  const float* xb = x + (long)b * T * C;
  const int Tb = vc_rows(lens, b, len_mul, T);
  if (t0 >= Tb) {                          // a tile beyond the utterance's end: the zeros of the result, nothing staged
    if (t0 + tid < T) out[(long)b * T + t0 + tid] = 0.f;
    return;
  }
  float acc = 0.f;
  for (int c0 = 0; c0 < C; c0 += 32) {
    __syncthreads();
    for (int e = tid; e < rows * 32; e += 256) {
      const int r = e >> 5, c = e & 31, t = t0 - half + r;
      float v = 0.f;
      if (t >= 0 && t < Tb && c0 + c < C) {
        v = xb[(long)t * C + c0 + c];
        v = v > 0.f ? v : v * slope;
      }
      xs[r * VP_PITCH + c] = v;
    }
    __syncthreads();
    const int cn = min(32, C - c0);
    for (int tap = 0; tap < k; ++tap) {
      const float* wr = w + (long)tap * C + c0;
      const float* xr = xs + (tid + tap) * VP_PITCH;
      for (int c = 0; c < cn; ++c) acc = fmaf(xr[c], wr[c], acc);
    }
  }
  const int t = t0 + tid;
  if (t < T) out[(long)b * T + t] = t < Tb ? tanhf(acc + bias[0]) : 0.f;
}

}  // namespace

extern "C" int ctts_vocoder_conv(const ctts_vconv_desc* dp, void* stream) {
  CTTS_REQUIRE(dp, "ctts_vocoder_conv: NULL descriptor");
  const ctts_vconv_desc& d = *dp;
  CTTS_REQUIRE(d.x && d.w && d.out, "ctts_vocoder_conv: x, w and out are required");
  CTTS_REQUIRE(d.B >= 1 && d.T >= 1 && d.Cin >= 1 && d.Cout >= 1 && d.k >= 1, "ctts_vocoder_conv: bad shape B=%d T=%d Cin=%d Cout=%d k=%d",
               d.B, d.T, d.Cin, d.Cout, d.k);
  VcParams p{};
  p.x = d.x; p.sxb = d.sxb; p.sxt = d.sxt; p.sxc = d.sxc;
  p.T = d.T; p.Cin = d.Cin; p.cin_pad = (d.Cin + 31) / 32 * 32; p.Cout = d.Cout;
  p.act_in = d.act_in; p.slope = d.slope;
  p.w = d.w; p.wp = d.w_planes; p.bias = d.bias; p.R = d.R; p.out = d.out; p.alpha = d.alpha; p.beta = d.beta;
  CTTS_REQUIRE(!d.lens || d.len_mul >= 1, "ctts_vocoder_conv: lens needs len_mul >= 1 (len_mul=%d)", d.len_mul);
  p.lens = d.lens; p.len_mul = d.len_mul;
  const int u = d.transposed_u;
  if (u == 0) {
    CTTS_REQUIRE(d.k % 2 == 1 && d.dil >= 1, "ctts_vocoder_conv: Conv1d needs an odd k and dil >= 1 (k=%d dil=%d)", d.k, d.dil);
    p.taps = d.k; p.dil = d.dil; p.in_off = -(d.k - 1) * d.dil / 2; p.row_off = 0; p.Mrows = d.T;
    p.N = d.Cout; p.u = 0; p.pad = 0; p.Tout = d.T;
  } else {
    CTTS_REQUIRE(u >= 1 && d.k % u == 0 && (d.k - u) % 2 == 0,
                 "ctts_vocoder_conv: ConvTranspose1d needs k %% u == 0 and (k - u) even (k=%d u=%d)", d.k, u);
    const int pad = (d.k - u) / 2, J = d.k / u;
    // q rows whose phases reach [0, T u): q u + r - pad >= 0 for some r < u, q u - pad < T u
    const int qlo = pad / u, qhi = d.T + (pad + u - 1) / u;
    p.taps = J; p.dil = 1; p.in_off = -(J - 1); p.row_off = qlo; p.Mrows = qhi - qlo;
    p.N = u * d.Cout; p.u = u; p.pad = pad; p.Tout = d.T * u;
  }
  p.mextra = p.Mrows - d.T;               // the grid is sized by the padded T: no host read of lens
  CTTS_REQUIRE((p.taps - 1) * p.dil <= VC_HALO_MAX, "ctts_vocoder_conv: halo (taps - 1) x dil = %d exceeds %d", (p.taps - 1) * p.dil,
               VC_HALO_MAX);
  const bool x6 = d.bf16_split != 0;
  CTTS_REQUIRE(!x6 || d.w_planes, "ctts_vocoder_conv: bf16_split needs w_planes");
  CTTS_REQUIRE(((uintptr_t)d.w & 15) == 0 && ((uintptr_t)d.w_planes & 15) == 0, "ctts_vocoder_conv: packed weights must be 16-byte aligned");
  CTTS_REQUIRE(d.out != d.x, "ctts_vocoder_conv: out must not alias x");
  p.vec = d.sxc == 1 && d.Cin % 4 == 0 && d.sxt % 4 == 0 && d.sxb % 4 == 0 && ((uintptr_t)d.x & 15) == 0;
  const int BN = p.N % 128 == 0 ? 128 : (p.N % 64 == 0 ? 64 : 32);
  dim3 grid((p.Mrows + VC_BM - 1) / VC_BM, (p.N + BN - 1) / BN, d.B);
  hipStream_t st = (hipStream_t)stream;
  if (x6) {
    if (BN == 128) hipLaunchKernelGGL((vconv_kernel<true, 128>), grid, dim3(256), 0, st, p);
    else if (BN == 64) hipLaunchKernelGGL((vconv_kernel<true, 64>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((vconv_kernel<true, 32>), grid, dim3(256), 0, st, p);
  } else {
    if (BN == 128) hipLaunchKernelGGL((vconv_kernel<false, 128>), grid, dim3(256), 0, st, p);
    else if (BN == 64) hipLaunchKernelGGL((vconv_kernel<false, 64>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((vconv_kernel<false, 32>), grid, dim3(256), 0, st, p);
  }
  CTTS_CHECK_LAUNCH("ctts_vocoder_conv");
  return 0;
}

static int vpost_launch(const char* what, const float* x, int B, int T, int C, int k, const float* w, const float* bias, float slope,
                        float* out, const int32_t* lens, int len_mul, void* stream) {
  CTTS_REQUIRE(x && w && bias && out && B >= 1 && T >= 1 && C >= 1 && k >= 1 && k % 2 == 1, "%s: bad arguments (B=%d T=%d C=%d k=%d)", what,
               B, T, C, k);
  const size_t lds = (size_t)(VP_ROWS + k - 1) * VP_PITCH * sizeof(float);
  CTTS_REQUIRE(lds <= 64 * 1024, "%s: k=%d too large", what, k);
  dim3 grid((T + VP_ROWS - 1) / VP_ROWS, B);
  hipLaunchKernelGGL(vpost_kernel, grid, dim3(256), lds, (hipStream_t)stream, x, T, C, k, w, bias, slope, out, lens, len_mul);
  CTTS_CHECK_LAUNCH(what);
  return 0;
}

extern "C" int ctts_vocoder_post(const float* x, int B, int T, int C, int k, const float* w, const float* bias, float slope, float* out,
                                 void* stream) {
  return vpost_launch("ctts_vocoder_post", x, B, T, C, k, w, bias, slope, out, nullptr, 1, stream);
}

extern "C" int ctts_vocoder_post_ragged(const float* x, int B, int T, int C, int k, const float* w, const float* bias, float slope,
                                        float* out, const int32_t* lens, int len_mul, void* stream) {
  CTTS_REQUIRE(lens && len_mul >= 1, "ctts_vocoder_post_ragged: lens and len_mul >= 1 are required (len_mul=%d)", len_mul);
  return vpost_launch("ctts_vocoder_post_ragged", x, B, T, C, k, w, bias, slope, out, lens, len_mul, stream);
}
