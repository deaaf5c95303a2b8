// HiFi-GAN V1 generator (reference hifigan/models.py:112-173) inference kernels, fp32 mode: every Conv1d of the network as ONE launch.
// The layer geometry (Conv1d / polyphase ConvTranspose1d, lens / len_mul), the epilogue walk and conv_post are vocoder_common.h's.
// Accepted, V1 or not: B, T, Cin, Cout >= 1; Conv1d with odd k and (k - 1) dil <= 64; ConvTranspose1d with k % u == 0, (k - u) even and
// k / u <= 65; any input strides and alignment (tests/test_vocoder_contract_gpu.py runs the edges of this contract).
//
// vconv_kernel: dilated Conv1d (stride 1, zero padding d (k - 1) / 2) and ConvTranspose1d as an implicit GEMM on the MFMA.
//   rows = (b, position p), N = output columns, K = taps x Cin.  A workgroup owns 128 positions of one utterance x BN columns.  For every
//   32-channel chunk of the input it stages its 128 rows PLUS the (taps - 1) x dil halo into LDS once (on-load leaky_relu, zero rows
//   outside [0, T)); every tap then reads a row-shifted view of that tile, so an input element is fetched and split once per tile and
//   chunk, not once per tap.  The weights arrive pre-packed [roundup(N, 128)][taps][roundup(Cin, 32)] (and, for the split arithmetic,
//   pre-split by ctts_split_planes: they are constant) and one tap's 32-deep K-block is staged per step, prefetched into registers
//   while the previous one is multiplied.
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
//   MelGAN (include/ctts.h, MelGAN block; melgan.py) runs on the same kernel body instantiated with MG = true: a row outside [0, Tb) is
//   staged from its reflection about the utterance's own ends instead of as zeros, and a 1x1 conv may continue its K loop over the
//   chunks of a second, un-activated input (the ResnetBlock's shortcut).  The MG = false instantiations are HiFi-GAN's, unchanged
//   (profiles/melgan_isa.md).
#include "vocoder_common.h"
#include "planes_common.h"

namespace {

typedef __bf16 vc_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int vc_u32x4 __attribute__((ext_vector_type(4)));

constexpr int VC_BM = 128;                 // positions per workgroup
constexpr int VC_AROWS = VC_BM + VC_HALO_MAX;
// X6 LDS: per operand three planes (hi | mid | lo) of 64-byte rows = 32 bf16 of one chunk; 16-byte chunks XOR-swizzled by (row >> 2) & 3
constexpr int VC_X6_APLANE = VC_AROWS * 64, VC_X6_BPLANE = 128 * 64;
// fp32 LDS: 128-byte rows = 32 floats; 16-byte chunks XOR-swizzled by (row >> 1) & 7
constexpr int VC_F32_A = VC_AROWS * 128, VC_F32_B = 128 * 128;
constexpr int VC_LDS_X6 = 3 * VC_X6_APLANE + 3 * VC_X6_BPLANE;     // 61,440 bytes
constexpr int VC_LDS_F32 = VC_F32_A + VC_F32_B;                     // 40,960 bytes

struct VcParams {
  VcGeom g;                                 // this field order keeps every kernel's register counts (profiles/vocoder_refactor_isa.md)
  const float* w; const uint16_t* wp; const float* R; float* out;
  const float* x; long sxb, sxt, sxc; int vec;
};

// MelGAN's two extensions (include/ctts.h, MelGAN block) ride behind the HiFi-GAN arguments: the MG = false kernels never see them
struct VcParamsMg {
  VcParams p;
  int reflect;                              // pad_mode: input rows outside [0, Tb) are read at their reflection
  const float* x2; long sx2b, sx2t; int Cin2, cin2_pad, vec2;     // second operand of a 1x1 conv (NULL: none), dense channels
};
__device__ __forceinline__ const VcParams& vc_base(const VcParams& a) { return a; }
__device__ __forceinline__ const VcParams& vc_base(const VcParamsMg& a) { return a.p; }

__device__ __forceinline__ int x6sw(int row, int c) { return c ^ ((row >> 2) & 3); }
__device__ __forceinline__ int f32sw(int row, int c) { return c ^ ((row >> 1) & 7); }

// MG = false: HiFi-GAN's kernels, the code they always were.  MG = true (P = VcParamsMg): reflect padding and the two-operand K loop.
template <bool X6, int BN, bool MG, class P>
__global__ __launch_bounds__(256, 2) void vconv_kernel(const P pa) {
  const VcParams& p = vc_base(pa);
  constexpr int NT = BN == 128 ? 2 : 1;
  constexpr int WAVES_N = BN / (32 * NT);             // 2, 2, 1
  constexpr int WAVES_M = 4 / WAVES_N;                // 2, 2, 4
  constexpr int MT = VC_BM / (32 * WAVES_M);          // 2, 2, 1
  constexpr int B_CHUNKS = X6 ? BN * 12 : BN * 8;     // 16-byte pieces of one staged weight K-block
  constexpr int B_PER_T = (B_CHUNKS + 255) / 256;
  __shared__ __attribute__((aligned(16))) unsigned char smem[X6 ? VC_LDS_X6 : VC_LDS_F32];
  unsigned char* sA = smem;
  unsigned char* sB = smem + (X6 ? 3 * VC_X6_APLANE : VC_F32_A);

  const VcGeom& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, m0 = blockIdx.x * VC_BM, col0 = blockIdx.y * BN;
  const int wm0 = (wave / WAVES_N) * (MT * 32), wn0 = (wave % WAVES_N) * (NT * 32);
  // ragged (include/ctts.h): the utterance's own length replaces T everywhere below; a tile at or beyond its end has nothing to do
  const int Tb = vc_rows(g.lens, b, g.len_mul, g.T), Mb = Tb + g.mextra, Toutb = g.u ? Tb * g.u : Tb;
  if (Tb == 0 || m0 >= Mb) return;
  const int p0 = g.row_off + m0;                      // position of tile row 0
  const int nchunks1 = g.cin_pad >> 5, taps = g.taps;
  int nchunks_ = nchunks1;
  long kp_ = (long)taps * g.cin_pad;
  if constexpr (MG) { nchunks_ += pa.cin2_pad >> 5; kp_ += pa.cin2_pad; }      // cin2_pad = 0 without x2; with it taps = 1
  const int nchunks = nchunks_;                       // K chunks: those of x, then those of x2
  const long kp = kp_;                                // packed weight row length
  const int arows = VC_BM + (taps - 1) * g.dil;
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
  // MG: under reflect a row outside [0, Tb) is read at its reflection (Tb the utterance's own); a chunk at or beyond nchunks1 is x2's
  auto stage_rows = [&](int chunk, const float* xs, long sxt, long sxc, int vec, int cin, int act) {
    const int c4 = tid & 7, cbase = chunk * 32 + c4 * 4;
    for (int i = tid >> 3; i < arows; i += 32) {
      int ti = p0 + g.in_off + i;
      if constexpr (MG) {
        if (pa.reflect) ti = ctts_reflect_index(ti, Tb);
      }
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (ti >= 0 && ti < Tb) {
        const float* src = xs + (long)ti * sxt;
        if (vec) {
          if (cbase < cin) {
            const float4 f = *reinterpret_cast<const float4*>(src + cbase);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (cbase + e < cin) v[e] = src[(long)(cbase + e) * sxc];
        }
        if (act) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * g.slope;
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

  auto stage_a = [&](int chunk) {
    if constexpr (MG) {
      if (chunk >= nchunks1) { stage_rows(chunk - nchunks1, pa.x2 + (long)b * pa.sx2b, pa.sx2t, 1, pa.vec2, pa.Cin2, 0); return; }
    }
    stage_rows(chunk, xb, p.sxt, p.sxc, p.vec, g.Cin, g.act_in);
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
      compute(tap * g.dil);
      if (tap + 1 < taps) {
        __syncthreads();
        store_b();
        __syncthreads();
      }
    }
  }

  vc_epilogue<MT, NT>(g, acc, b, m0, col0, wm0, wn0, l31, h, Mb, Toutb,
                      [R = p.R, out = p.out, alpha = g.alpha, beta = g.beta](long idx, float v) {
    if (R) v += R[idx];
    v *= alpha;
    if (beta != 0.f) v = beta * out[idx] + v;
    out[idx] = v;
  });
}

template <bool MG, class P>
void vconv_launch(bool x6, int BN, dim3 grid, hipStream_t st, const P& p) {
  if (x6) {
    if (BN == 128) hipLaunchKernelGGL((vconv_kernel<true, 128, MG, P>), grid, dim3(256), 0, st, p);
    else if (BN == 64) hipLaunchKernelGGL((vconv_kernel<true, 64, MG, P>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((vconv_kernel<true, 32, MG, P>), grid, dim3(256), 0, st, p);
  } else {
    if (BN == 128) hipLaunchKernelGGL((vconv_kernel<false, 128, MG, P>), grid, dim3(256), 0, st, p);
    else if (BN == 64) hipLaunchKernelGGL((vconv_kernel<false, 64, MG, P>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((vconv_kernel<false, 32, MG, P>), grid, dim3(256), 0, st, p);
  }
}

// the one launcher behind ctts_vocoder_conv (m == NULL) and ctts_vocoder_conv_melgan (m: its descriptor, d = m->conv)
int vconv_run(const ctts_vconv_desc& d, const ctts_vconv_melgan_desc* m, void* stream) {
  CTTS_REQUIRE(d.x && d.w && d.out, "ctts_vocoder_conv: x, w and out are required");
  VcParams p{};
  int BN;
  if (int rc = vc_geometry("ctts_vocoder_conv", d.B, d.T, d.Cin, d.Cout, d.k, d.dil, d.transposed_u, d.lens, d.len_mul, p.g, BN)) return rc;
  p.g.act_in = d.act_in; p.g.slope = d.slope; p.g.alpha = d.alpha; p.g.beta = d.beta; p.g.bias = d.bias;
  p.x = d.x; p.sxb = d.sxb; p.sxt = d.sxt; p.sxc = d.sxc;
  p.w = d.w; p.wp = d.w_planes; p.R = d.R; p.out = d.out;
  const bool x6 = d.bf16_split != 0;
  CTTS_REQUIRE(!x6 || d.w_planes, "ctts_vocoder_conv: bf16_split needs w_planes");
  CTTS_REQUIRE(((uintptr_t)d.w & 15) == 0 && ((uintptr_t)d.w_planes & 15) == 0, "ctts_vocoder_conv: packed weights must be 16-byte aligned");
  CTTS_REQUIRE(d.out != d.x, "ctts_vocoder_conv: out must not alias x");
  p.vec = d.sxc == 1 && d.Cin % 4 == 0 && d.sxt % 4 == 0 && d.sxb % 4 == 0 && ((uintptr_t)d.x & 15) == 0;
  const dim3 grid = vc_grid(p.g, VC_BM, BN, d.B);
  hipStream_t st = (hipStream_t)stream;
  CTTS_REQUIRE(!m || m->pad_mode == 0 || m->pad_mode == 1, "ctts_vocoder_conv_melgan: pad_mode must be 0 (zero) or 1 (reflect), got %d",
               m ? m->pad_mode : 0);
  if (!m || (m->pad_mode == 0 && !m->x2)) {
    vconv_launch<false>(x6, BN, grid, st, p);
  } else {                                   // reflect padding and / or the second operand of a 1x1 conv
    CTTS_REQUIRE(d.transposed_u == 0, "ctts_vocoder_conv_melgan: pad_mode = 1 and x2 are for Conv1d only (transposed_u=%d)", d.transposed_u);
    CTTS_REQUIRE(!m->pad_mode || d.T > (d.k - 1) * d.dil / 2,
                 "ctts_vocoder_conv_melgan: reflection needs T > dil (k - 1) / 2 (T=%d k=%d dil=%d)", d.T, d.k, d.dil);
    VcParamsMg q{};
    q.p = p; q.reflect = m->pad_mode;
    if (m->x2) {
      CTTS_REQUIRE(d.k == 1 && m->Cin2 >= 1, "ctts_vocoder_conv_melgan: x2 needs k == 1 and Cin2 >= 1 (k=%d Cin2=%d)", d.k, m->Cin2);
      CTTS_REQUIRE(d.out != m->x2, "ctts_vocoder_conv_melgan: out must not alias x2");
      q.x2 = m->x2; q.sx2b = m->sx2b; q.sx2t = m->sx2t; q.Cin2 = m->Cin2; q.cin2_pad = (m->Cin2 + 31) / 32 * 32;
      q.vec2 = m->Cin2 % 4 == 0 && m->sx2t % 4 == 0 && m->sx2b % 4 == 0 && ((uintptr_t)m->x2 & 15) == 0;
    }
    vconv_launch<true>(x6, BN, grid, st, q);
  }
  CTTS_CHECK_LAUNCH("ctts_vocoder_conv");
  return 0;
}

}  // namespace

extern "C" int ctts_vocoder_conv(const ctts_vconv_desc* dp, void* stream) {
  CTTS_REQUIRE(dp, "ctts_vocoder_conv: NULL descriptor");
  return vconv_run(*dp, nullptr, stream);
}

extern "C" int ctts_vocoder_conv_melgan(const ctts_vconv_melgan_desc* dp, void* stream) {
  CTTS_REQUIRE(dp, "ctts_vocoder_conv_melgan: NULL descriptor");
  return vconv_run(dp->conv, dp, stream);
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

extern "C" int ctts_vocoder_post_reflect(const float* x, int B, int T, int C, int k, const float* w, const float* bias, float slope,
                                         float* out, const int32_t* lens, int len_mul, void* stream) {
  return vpost_launch<float, true>("ctts_vocoder_post_reflect", x, B, T, C, k, w, bias, slope, out, lens, lens ? len_mul : 1, stream);
}
