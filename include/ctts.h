/* ctts.h - C ABI of libctts_hip.so: the MI355X (gfx950) kernels behind the CompTransTTS hot path.
 *
 * Conventions:
 *   - every pointer is a raw DEVICE pointer (torch `tensor.data_ptr()`), shapes/strides are
 *     explicit, `stream` is a hipStream_t passed as void* (PyTorch's current stream);
 *   - functions return 0 on success, <0 on error (ctts_last_error() gives the text);
 *     no C++ exception crosses the ABI; the library never allocates caller-visible memory,
 *     all calls are asynchronous and stream-ordered (graph-capturable);
 *   - layouts are channel-last / row-major: activations are [B, T, C] (C contiguous).
 *
 * Each entry point names the reference code it replaces (paths relative to the reference
 * repository keonlee9420/Comprehensive-Transformer-TTS).  The reference has no FFI of its
 * own (it is pure Python on torch ops); INTEGRATION.md shows the ctypes binding.
 */
#ifndef CTTS_H
#define CTTS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* ctts_last_error(void);
int ctts_version(void);

/* ---------------------------------------------------------------------------------------
 * General fp32 MFMA GEMM with implicit-im2col ("conv") operand views and fused epilogue.
 *   C[m,n] = epi( alpha * (sum_k opA[m,k] * opB[k,n] + bias[n]) )
 *   epi(v) = rowscale[m] * (R[m,n] + drop(act(v)))   (Z, if given, receives v)
 * opA[m,k] = A[m*lda + k] (a_kc=1) or A[k*lda + m] (a_kc=0); opB[k,n] = B[n*ldb + k] (b_kc=1)
 * or B[k*ldb + n] (b_kc=0).  Replaces torch.nn.functional.linear / conv1d / bmm call sites:
 *   - Conv1d(k=9) FFN            model/transformers/transformer_fs2.py:220-239
 *   - in/out projections, QK^T, PV  (F.multi_head_attention_forward)  transformer_fs2.py:385-394
 *   - predictor Conv1d(k=3,5)    model/modules.py:1299-1356
 *   - mel_linear                 model/CompTransTTS.py:133
 *   - PostNet Conv1d(k=5)        model/modules.py:140-148
 *   - STFT-as-conv1d + mel matmul  audio/stft.py:72-80,177
 * Conv view: rows of the operand are (b,t) pairs with t = row % conv_T; element (row, kk)
 * reads X[(row - conv_pad)*ld + kk] and is zero unless 0 <= t - conv_pad + kk/conv_cin < conv_T.
 * The viewed operand is dense, ld == conv_cin (a K index runs on into the next rows; with another ld the kernel families address
 * different elements), and made of whole utterances: its row count (M, or K with conv_on_b) is a multiple of conv_T, because the
 * zero test looks at t alone.
 * Rules every kernel family follows (tests/gemm_restate64.py restates the descriptor in float64, tests/test_gemm_contract_gpu.py holds
 * every route kind to it): bias, R, Z and rowscale are NOT batched - every batch reads R[m*ldr + n] and rowscale[m] and stores
 * Z[m*ldz + n]; the dropout element index is batch*M*N + m*N + n with the descriptor's M and N, in 32 bits (wrapping); cells of C and
 * Z outside the [M, N] block of a batch (columns N .. ld-1, other rows, the gaps between batches) are never written.
 */
typedef struct ctts_gemm_desc {
  const float* A; const float* B; float* C;
  int32_t M, N, K;
  int64_t lda, ldb, ldc;
  int32_t a_kc, b_kc;
  int32_t nb0, nb1;                       /* batch = nb0*nb1 (blockIdx.z = z0*nb1+z1); 1,1 = none   */
  int64_t sA0, sA1, sB0, sB1, sC0, sC1;   /* element strides per batch level                          */
  const int32_t* lens;                    /* [nb0] valid length per z0, or NULL                       */
  int32_t lim_m, lim_n, lim_k;            /* clamp that dim to lens[z0]                               */
  int32_t conv_T, conv_pad, conv_cin, conv_on_b; /* conv_T=0: plain; conv_on_b=1 applies to B (b_kc=0) */
  int32_t split_k;                        /* >1: C += alpha * A B, K cut into <= split_k pieces summed in a FIXED order through sk_ws (no atomics, no epilogue:
                                             pass no bias / act / Z / dropout / R / rowscale with it - the tile kernels ignore them, the persistent ones may not) */
  float alpha;
  const float* bias;                      /* [N] or NULL                                              */
  float* Z; int64_t ldz;                  /* optional store of the pre-activation                     */
  int32_t act;                            /* 0 none, 1 relu, 2 gelu(erf), 3 tanh, 4 swish             */
  float p_drop; const uint64_t* seed; uint32_t drop_offset;   /* inverted dropout after act           */
  const float* R; int64_t ldr;            /* residual added after dropout                             */
  const float* rowscale;                  /* [M] multiplied last (non-pad mask), or NULL              */
  /* Padded-row skipping.  Rows (of C for a_kc=1, of the reduction dim for the TN layout) are (b,t) pairs,
   * t = row % row_T; rows with t >= row_lens[b] + row_halo are padding whose result is defined as ZERO:
   * whole output tiles of such rows are zero-filled without touching the operands (a_kc=1), and K-blocks
   * of such rows are skipped in weight-gradient reductions (a_kc=0, b_kc=0).  NULL = off.
   * Only WHOLE tiles (tile_m rows of the kernel that runs, ctts_gemm_route) and whole K-blocks are skipped; a padded row that shares a
   * tile with a live row is computed from the operands like any other.  It is the CALLER's duty to pass operands whose result is zero
   * there: the rows of A beyond length + halo are zero (and no bias, or a zero rowscale, reaches them) - then every padded row of C
   * (and of a stored Z) is zero whichever kernel runs.  For the TN layout the rows of A (dZ) in the padding MUST be exactly zero:
   * the two-group kernel (kind BUF_K2) skips nothing and multiplies them.  With split_k > 1 a skipped tile adds nothing to C, or
   * stores zero under split_overwrite. */
  const int32_t* row_lens; int32_t row_T; int32_t row_halo;
  /* Optional m-tile schedule for row_lens launches (ctts_row_tile_map, 64-row tiles): tile_map[0] = number of ACTIVE m-tiles,
   * tile_map[1..] = m-tile indices, active ones first.  Workgroup b then works on m-tile tile_map[1 + b / tiles_n] and n-tile
   * b % tiles_n: the active tiles occupy the first workgroup ids, so the hardware's round-robin placement spreads them evenly over
   * the 8 XCDs (a fixed permutation leaves a +-10 % imbalance of active tiles per XCD), and each XCD only sees tiles_n / 8 weight
   * panels.  NULL = built-in scrambled order.
   * On a launch with per-batch length limits (lens and a lim_*; no row_lens, split_k <= 1) tile_map is instead a BATCH TILE PLAN
   * (ctts_batch_tile_map, built for the same nb0, nb1, M, N, lim_* and split_overwrite): the workgroup with linear id
   * blockIdx.z * gridDim.x + blockIdx.x works on the (batch, tile) the plan lists there - active tiles first, dealt evenly by work
   * over the compute units.  Only the 64 x 64 buffer kernel follows one (ctts_gemm refuses it on any other route); a plan built for
   * another geometry is not followed (plain order).  Results do not depend on it.  NULL = plain order. */
  const int32_t* tile_map;
  /* with tile_map: n-tiles per XCD group (0 = plain order).  g > 0 (tiles_n % g == 0, tiles_n / g in {1,2,4,8}): XCD x works on the g
   * n-tiles of group x % (tiles_n/g) and on every (8*g/tiles_n)-th scheduled m-tile - trades weight-panel against activation-tile
   * footprint in the XCD's 4 MiB L2. */
  int32_t tile_group_n;
  /* Optional softmax-backward fusion (attention): C = E * (alpha * acc - rowsub[row]) with E laid out exactly like C (same ldc and
   * batch strides) and rowsub indexed [batch * M + row]:  dS = P * (dP - D), D = rowsum(dO * O), straight out of the dP = dO V^T GEMM -
   * no separate pass over the [T,T] maps.  NULL = off; not combinable with bias / act / dropout / R / rowscale / split_k.  E is addressed
   * from its own pointer (batch strides, m*ldc + n): an element offset folded into the C pointer is not applied to it; rowsub uses the
   * descriptor's M also where lens cut a batch shorter. */
  const float* E; const float* rowsub;
  /* Workspace (ctts_workspace_bytes() bytes, zero-filled ONCE by the caller, private to the stream the launch goes to: launches that
   * share it must be stream-ordered; every kernel leaves its flag / ticket words at zero).  REQUIRED when split_k > 1: the partial tiles
   * of the K pieces are written to it and summed in split order by the workgroup that finishes last - bit-reproducible, unlike float
   * atomics in arrival order.  It also enables the persistent stream-K kernel (csrc/gemm_sk.hip): with it, large unbatched GEMMs
   * run on a persistent grid that cuts the (tile, K-block) space evenly over the CUs and sums cut tiles in a fixed order; split_k > 1
   * then only means "C += alpha * A B" (no atomics).  NULL = tile-per-workgroup kernels only. */
  void* sk_ws; int64_t sk_ws_bytes;
  /* epi_bwd != 0: the epilogue is the BACKWARD of a previous layer's forward epilogue - Z is then an INPUT (that layer's stored
   * pre-activation, laid out like C with ldz) and  C = drop_mask(seed, drop_offset, m*N+n)/(1-p) * act'(Z) * alpha * acc : the data-gradient
   * GEMM of layer k+1 hands layer k its dZ directly, no separate pass over the [M,N] gradient.  Excludes bias / R / rowscale / E / split_k. */
  int32_t epi_bwd;
  /* Deferred split-K (split_k > 1, tile kernels): the partial matrices P_0 .. P_count-1 ([M, N rounded up to 4] each, `stride` floats apart -
   * ctts_gemm_split_plan) are written HERE and left for the caller, who adds them in order later with ctts_partial_sums - the second
   * halves of all weight gradients of a backward stage in one launch instead of one reduce launch per GEMM.  NULL = the library adds them
   * itself (through sk_ws) before ctts_gemm returns control of the stream. */
  float* split_out; int64_t split_out_floats;
  /* "Write everything": every element of the [M, N] block of every batch is WRITTEN, zero where the per-batch limits (lens) or a whole
   * tile of padded rows (row_lens) leave nothing to compute - the caller needs no pre-zeroed C (one fill launch per attention product /
   * convolution data gradient saved).  With split_k > 1 (library-side sum only) this also turns C += alpha * A B into C = alpha * A B;
   * with split_k <= 1 it only adds the zeros outside the limits of a batched, length-limited launch. */
  int32_t split_overwrite;
  /* Arithmetic of the large launches (a DESCRIPTOR field since round 5; it used to be the process-wide ctts_gemm_bf16_split_enable
   * switch, which a captured graph ignored and two models in one process could not set differently):
   *   0 = fp32 MFMA only (v_mfma_f32_32x32x2_f32: every product an exact fp32 product) - what a zero-initialised descriptor gets;
   *   1 = launches that qualify by shape and size may run on the BF16 matrix pipe with the six-term operand split described at
   *       ctts_gemm_takes_bf16_split below (fp32-class results);
   *   2 = as 1 without the size thresholds (parity tests of small launches);
   *   3 = REDUCED precision, opt-in ("amp": reference train.py:59,104 amp.autocast): launches the plane kernels take (A_planes / B_planes
   *       given and eligible) use the hi pieces only - operands rounded to bf16 (round-to-nearest-even), ONE MFMA term, fp32 accumulate:
   *       the result equals the product of the bf16-rounded operands up to fp32 summation; every other launch is treated as 1;
   *   4 = as 3 without the size thresholds. */
  int32_t bf16_split;
  /* Optional PRE-SPLIT operands (ctts_split_planes): A_planes / B_planes hold the exact three-way bf16 split of the SAME fp32 matrices
   * A / B point to, in the K-block-interleaved layout [rows][ld / 32][3][32] (bf16 bit patterns): piece q (0 hi, 1 mid, 2 lo) of element
   * (row, k) at planes[row * 3 * ld + (k / 32) * 96 + q * 32 + k % 32] - the three pieces of one 32-deep K-block of a row are 192
   * contiguous bytes; same ld as the fp32 operand, ld % 32 == 0, 16-byte aligned.  With both given (bf16_split >= 1, a_kc = b_kc = 1,
   * unbatched, sk_ws given) the persistent plane kernel (csrc/gemm_pl.hip) moves the pieces to LDS by DMA and its main loop is
   * ds_read + MFMA only: no split arithmetic in the GEMM, every operand element split ONCE per tensor instead of once per tile that
   * stages it.  The SAME row-major plane sets serve the TN layout (a_kc = b_kc = 0: weight gradients C[m][n] (+)= alpha * sum_k
   * A[k][m] B[k + tap - pad][c], conv view on B): csrc/gemm_plw.hip DMAs 32-row K-blocks into LDS as they lie and transposes with
   * ds_read_b64_tr_b16 - pass the planes of dZ (made for the data gradient) as A_planes and of x (made for the forward) as B_planes;
   * split_k > 1 without split_overwrite adds into C in place (M % 128 == 0, N % 256 == 0, conv_cin % 256 == 0, no epilogue terms).
   * A / B must stay valid: descriptors the plane kernels do not take (ctts_gemm_takes_planes) run on the other kernels from A / B. */
  const uint16_t* A_planes;
  const uint16_t* B_planes;
  /* Optional plane set of the OUTPUT (round 6): with epi_bwd != 0 on the weight-stationary K = 256 kernel (ctts_gemm_takes_weight_stationary)
   * the epilogue writes the exact three-way bf16 split of every C element it stores into C_planes as well ([M][ldc / 32][3][32], ldc % 32
   * == 0, N % 32 == 0, 16-byte aligned; zeros in wholly padded tiles like C itself) - bit-identical to ctts_split_planes(C).  The dZ a
   * data-gradient GEMM hands the previous layer then arrives with the operand planes that layer's own data- and weight-gradient launches
   * read (transformer_fs2.py:220-239: ffn_2 -> ffn_1).  Launches on any other kernel IGNORE the field: ask first. */
  uint16_t* C_planes;
} ctts_gemm_desc;

int ctts_gemm(const ctts_gemm_desc* d, void* stream);
/* 1 (+ *count, *stride) when ctts_gemm would run `d` as a split-K launch whose partials the caller may keep (split_out); else 0.
 * For a descriptor with a K-contiguous A (NT / NN) the answer IGNORES A_planes / B_planes: the plane forward kernel takes split_k > 1
 * with split_overwrite as a plain overwrite and writes no partials - do not defer such a launch (ask ctts_gemm_route). */
int ctts_gemm_split_plan(const ctts_gemm_desc* d, int32_t* count, int64_t* stride);
/* Which kernel ctts_gemm would run `d` on (csrc/gemm.hip gemm_route - the one place that orders the kernel families; no launch).  Same
 * validation as ctts_gemm: an invalid descriptor gets its error (< 0), not a route.  tile_m x tile_n: the workgroup tile; split_k: the
 * number of K ranges that write partial matrices, as it will run (lowered until the partials fit; 1 for every kernel that finishes its
 * sum itself); k_granule: the multiple of K elements a split's range is rounded to.  kind NONE: M or N is 0, nothing is launched. */
typedef enum ctts_gemm_kind {
  CTTS_GEMM_NONE = 0,
  CTTS_GEMM_PLANES, CTTS_GEMM_PLANES_WGRAD,          /* gemm_pl.hip, gemm_plw.hip: pre-split bf16 planes */
  CTTS_GEMM_WEIGHT_STATIONARY,                       /* gemm_ws.hip: K = 256 */
  CTTS_GEMM_X6,                                      /* gemm.hip: NT, operands split inside the kernel */
  CTTS_GEMM_STREAM_K,                                /* gemm_sk.hip: persistent */
  CTTS_GEMM_X6TN,                                    /* from here on: tile-per-workgroup kernels of gemm.hip (ordered split-K partials) */
  CTTS_GEMM_SCALAR64, CTTS_GEMM_BUF128, CTTS_GEMM_BUF_K2, CTTS_GEMM_BUF_NARROW, CTTS_GEMM_BUF64, CTTS_GEMM_VEC128, CTTS_GEMM_VEC64
} ctts_gemm_kind;
typedef struct ctts_gemm_route_info { int32_t kind, tile_m, tile_n, split_k, k_granule; } ctts_gemm_route_info;
int ctts_gemm_route(const ctts_gemm_desc* d, ctts_gemm_route_info* info);
/* Data-gradient operands of many Conv1d layers in one launch: for every task dst[ci][kk][co] = src[co][k-1-kk][ci], src = the GEMM-major
 * forward weight [Cout][K][Cin] (what ctts_conv_weight_repack mode 4 does for one layer; 32 x 32 tiles through LDS, both sides
 * coalesced).  `tasks` is a HOST array.  The weights are constant during a step: trainer.TrainStep calls this once before the forward. */
typedef struct ctts_repack_task { const float* src; float* dst; int32_t cout, cin, k; } ctts_repack_task;
int ctts_conv_dgrad_weights(const ctts_repack_task* tasks, int ntasks, void* stream);
/* y = rowscale[row] * dropout(x + alpha * table[pos[row]]): positional-embedding add of the fs2 stacks and predictors
 * (`x + self.pos_embed_alpha * self.embed_positions(x)` + F.dropout + non-pad mask, transformer_fs2.py:41-52,113-119, modules.py:1349-1351)
 * as one launch each way; pos from ctts_positions, table [n_pos, C] row-major, alpha a device scalar or NULL (= 1), rowscale / dropout
 * optional.  Backward: dx = rowscale * dropmask * dy; dalpha (optional, (+)= by `accumulate`) = sum of dx * table[pos] (ordered sum, ws). */
int ctts_posembed_fwd(const float* x, const int32_t* pos, const float* table, const float* alpha, const float* rowscale, float* y,
                      int64_t rows, int C, float p_drop, const uint64_t* seed, uint32_t drop_offset, void* stream);
int ctts_posembed_bwd(const float* dy, const int32_t* pos, const float* table, const float* rowscale, float* dx, float* dalpha,
                      int64_t rows, int C, float p_drop, const uint64_t* seed, uint32_t drop_offset, int accumulate, void* ws, void* stream);
/* Deferred ordered reductions, many per launch: for every task  dst[i] += alpha * (src[i] + src[stride + i] + ... + src[(count-1)*stride + i]),
 * i < n, partials added in index order (bit-reproducible).  `tasks` is a HOST array (copied into kernel arguments, 24 tasks per launch).
 * Producers: ctts_gemm with split_out; ctts_colsum / ctts_weighted_colsum / ctts_epilogue_bwd / ctts_layernorm_bwd with `parts`
 * (ctts_reduce_parts(kind, rows, C) partial rows of C floats - 2 C for kind 3 - written, nothing else). */
typedef struct ctts_psum_task { const float* src; float* dst; int64_t n; int64_t stride; int32_t count; float alpha; } ctts_psum_task;
int ctts_partial_sums(const ctts_psum_task* tasks, int ntasks, void* stream);
int ctts_reduce_parts(int kind, int64_t rows, int C);     /* kind 0 colsum, 1 weighted_colsum, 2 epilogue_bwd bias, 3 layernorm_bwd; 0 = no deferred mode */
/* Size of the per-stream workspace shared by ctts_gemm (sk_ws) and by every entry point below that takes a `ws` argument (ordered
 * cross-workgroup reductions: column sums, LayerNorm / BatchNorm parameter sums, loss sums).  `ws` = NULL is legal for those: the
 * reduction then runs on ONE workgroup per column block (slow, still deterministic).  ctts_gemm_workspace_bytes is the older name. */
size_t ctts_workspace_bytes(void);
size_t ctts_gemm_workspace_bytes(void);
/* Error word of the stream-K hand-off in a workspace (0 = clean; n > 0: an owner gave up waiting for workgroup n - 1 and the launch's
 * result is invalid).  DEVICE pointer to one uint32 inside `ws`: copy it to the host (asynchronously, e.g. every N steps) and raise. */
const uint32_t* ctts_workspace_error_word(const void* ws);
/* out[b] = XCC_ID (the XCD) workgroup b of an nblocks-wide launch ran on.  The persistent stream-K kernel assumes b % 8 (the default SPX
 * dispatch of an MI355X): callers verify once per device before handing ctts_gemm a workspace. */
int ctts_xcd_probe(int32_t* out, int nblocks, void* stream);
/* 1 when the persistent stream-K kernel is ELIGIBLE for this descriptor, asked on its own (sk_ws given, shape / alignment eligible,
 * enough tiles for the grid), else 0 - kernels that ctts_gemm asks earlier (planes, weight-stationary, x6) may still take the launch:
 * ctts_gemm_route names the kernel that runs.  Callers that otherwise split the reduction (split_k > 1 + zero fill) ask first: the
 * persistent kernel balances the reduction itself and wants split_k = 1. */
int ctts_gemm_takes_persistent(const ctts_gemm_desc* d);
/* Switch for the weight-stationary K = 256 kernel (csrc/gemm_ws.hip; default on, env CTTS_WS=0 turns it off): returns the previous
 * setting.  Process-wide, not thread-safe - for parity tests and A/B timing (same descriptor on both kernel families). */
int ctts_gemm_ws_enable(int on);
/* 1 when the weight-stationary kernel is ELIGIBLE for this descriptor, asked on its own (no launch; only the plane kernels are asked
 * before it - ctts_gemm_route names the kernel that runs).  0 for an `act` outside 0 / 1 / 2 / 4: the kernel has no instantiation for
 * tanh or for undefined codes (before ABI version 2 the answer for an undefined code was 1 although the tile kernels ran the launch). */
int ctts_gemm_takes_weight_stationary(const ctts_gemm_desc* d);
/* fp32 GEMM on the BF16 matrix pipe (ctts_gemm_desc.bf16_split >= 1; csrc/gemm.hip gemm_x6_kernel / gemm_x6tn_kernel, csrc/gemm_pl.hip
 * gemm_pl_kernel): large unbatched NT launches (both operands K-contiguous, conv view on A allowed, N a multiple of 128, split_k <= 1)
 * and large unbatched TN launches (weight gradients: both operands reduction-major, conv view on B allowed, M and N multiples of 128,
 * K >= 2048, any split_k) form every fp32 product from six v_mfma_f32_32x32x16_bf16 terms of the EXACT three-way bf16 split of both
 * operands (x = hi + mid + lo, each piece the round-to-nearest-even of what is left: hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi),
 * accumulated in fp32 - fp32-class results (exact wherever the fp32 result is exact; the three dropped cross terms are <= 2^-24 of a
 * product - one fp32 rounding - and 2^-29 in the median; error against float64 as the fp32-MFMA kernels' on the same launches) at up
 * to 16/6 of the fp32-MFMA rate.
 * DOMAIN (tests/test_kernels_gpu.py::test_bf16_split_domain_*):
 *   - finite operands with 2^-100 <= |x| < 3.396e38 (or x = 0): as stated above;
 *   - |x| < 2^-100: the lo (then mid) piece leaves the normal range of bf16 and is flushed by the matrix pipe: the product keeps >= 16
 *     (then >= 8) significant bits - an absolute error below 2^-116 |y| per product, far under the fp32 rounding of any sum that also
 *     holds a normal-sized term;
 *   - 3.396e38 <= |x| <= FLT_MAX (the top 0.2 % of the fp32 range, where hi would round to infinity): the pre-split path
 *     (ctts_split_planes) clamps hi to the largest bf16 and stays exact; the kernels that split inside the GEMM (x6 / x6tn) treat
 *     such an operand like an infinity;
 *   - an infinite or NaN operand makes every output element it contributes to NON-FINITE (NaN where fp32 arithmetic would give
 *     +-inf: inf * 0-piece = NaN), elements it does not contribute to are unaffected - the finite / non-finite pattern of the result
 *     equals the fp32-MFMA kernels', which is what overflow diagnostics (isfinite checks, GradScaler) look at.
 * Both read the route: ctts_gemm_takes_bf16_split: 1 when ctts_gemm WILL run this descriptor on the in-kernel-split kernels (kind X6 /
 * X6TN; no launch); ctts_gemm_takes_planes: 1 when it will run it on a plane kernel (kind PLANES: NT; PLANES_WGRAD: TN).  Unlike
 * ctts_gemm_route they do not validate the descriptor. */
int ctts_gemm_takes_bf16_split(const ctts_gemm_desc* d);
int ctts_gemm_takes_planes(const ctts_gemm_desc* d);
/* Exact three-way bf16 split of fp32 matrices, many per launch: for every task and element (r, c), c < cols (cols % 32 == 0, ld % 32 == 0,
 * src and dst 16-byte aligned): x = src[r * ld + c] -> dst[r * 3 * ld + (c / 32) * 96 + q * 32 + c % 32] = bf16 bits of piece q (the
 * layout of ctts_gemm_desc.A_planes), hi = RNE_bf16(x) (clamped to +-bf16 max when a finite x would round to infinity),
 * mid = RNE_bf16(x - hi), lo = x - hi - mid (exact); for x = +-inf / NaN: hi = x, mid = lo = 0.  dst holds rows * 3 * ld bf16.
 * `tasks` is a HOST array.  HBM-bound: 4 bytes read + 6 written per element. */
typedef struct ctts_split_task { const float* src; uint16_t* dst; int64_t rows, cols, ld; } ctts_split_task;
int ctts_split_planes(const ctts_split_task* tasks, int ntasks, void* stream);

/* out[b,h,t] = sum_d a[b,t,h*dh+d] * b[b,t,h*dh+d]   (a, b [B,T,H*dh] channel-last; the D vector of the fused softmax backward). */
int ctts_rowdot_heads(const float* a, const float* b, float* out, int B, int T, int H, int dh, void* stream);

/* out[c] (+)= scale * sum_r w[r] * x[r,c] (x [rows,C] dense): the weight gradient of a one-output Linear - the N = 1 heads of the
 * duration / energy predictors (modules.py:1296,1349) - as one streaming pass instead of a degenerate 1 x C GEMM. */
int ctts_weighted_colsum(const float* x, const float* w, float* out, int64_t rows, int C, float scale, int accumulate, void* ws, float* parts,
                         void* stream);

/* Backward of the ctts_gemm epilogue in one pass over dY [rows,C]:  gm = dY * rowscale[row] (optional output = gradient of the
 * residual R), dZ = gm * dropout_mask(seed, drop_offset, element) / (1-p) * act'(Z) (act as in ctts_gemm_desc; Z NULL or act 0: factor 1),
 * dbias[c] (+)= bias_scale * sum_rows dZ[.,c] (optional; bias_scale = the epilogue's alpha).  Any of rowscale, z, gm, dbias may be NULL. */
int ctts_epilogue_bwd(const float* dy, const float* rowscale, const float* z, float* dz, float* gm, float* dbias, int64_t rows, int C,
                      int act, float p_drop, const uint64_t* seed, uint32_t drop_offset, float bias_scale, int accumulate_bias,
                      void* ws, float* parts, void* stream);

/* m-tile schedule for padded-row skipping (see ctts_gemm_desc.tile_map): a 64-row tile is inactive when all its rows (b,t) belong to one
 * utterance b and t >= row_lens[b] + row_halo.  tile_map: 1 + ceil(M/64) int32. */
int ctts_row_tile_map(const int32_t* row_lens, int row_T, int row_halo, int M, int32_t* tile_map, void* stream);

/* Batch tile plan for launches with per-batch length limits (see ctts_gemm_desc.tile_map; csrc/batch_plan.h): a permutation of the
 * (batch, 64 x 64 tile) items of nb0 x nb1 batches of [M, N] outputs, built on the device from lens [nb0] (no host sync: capturable;
 * rebuild it when the lengths change).  Active tiles (inside the batch's limits) come first, sorted by their K-blocks and dealt in snake
 * order over the compute units; then, with write_all (the launch's split_overwrite), the tiles the launch zero-fills.  tile_map[0] =
 * active tiles, [1] = listed tiles, [2] = all tiles, [3] = geometry key, then one item per workgroup id.  One plan serves every launch
 * with the same nb0, nb1, M, N, K, lim_* and write_all, whatever its operand layout.
 * ctts_batch_tile_map_ints: the int32 the plan takes, or 0 when these batches do not fit one (launch without a plan then). */
size_t ctts_batch_tile_map_ints(int nb0, int nb1, int M, int N);
int ctts_batch_tile_map(const int32_t* lens, int nb0, int nb1, int M, int N, int K, int lim_m, int lim_n, int lim_k, int write_all,
                        int32_t* tile_map, size_t map_ints, void* stream);

/* Conv1d weight repack: w[Cout][Cin][K] (reference nn.Conv1d layout) ->
 *   mode 0: wf[Cout][K][Cin]                 (forward implicit-GEMM B operand)
 *   mode 1: wd[Cin][K][Cout], taps flipped   (data-gradient implicit-GEMM B operand)
 *   mode 2: inverse of mode 0 (wgrad result [Cout][K][Cin] -> [Cout][Cin][K])
 *   mode 3: as mode 2 but ADDED to dst (gradient accumulation straight into param.grad)
 *   mode 4: wd from a weight that is already stored GEMM-major, src = wf[Cout][K][Cin] (the layout this package keeps its own Conv1d
 *           parameters in - exposed with reference shape [Cout,Cin,K] through strides - so that forward and wgrad need no repack)  */
int ctts_conv_weight_repack(const float* src, float* dst, int cout, int cin, int k, int mode, void* stream);

/* ---------------------------------------------------------------------------------------
 * LengthRegulator / dur_to_mel2ph (model/modules.py:1216-1249, utils/tools.py:577-628).
 * ctts_lr_index: per batch row, prefix-sum of max(trunc(dur),0) by wavefront scan, then
 *   mel2ph[b,t] = 1 + #{i : cum[i] <= t} for t < min(total, Tm) else 0;  mel_len[b] = total
 *   (un-cropped).  dur_is_float selects float32 vs int64 input; round_mode 0 = trunc (LR),
 *   1 = round-half-even (dur_to_mel2ph); pad[b,i] != 0 zeroes that duration (dur_padding).
 *   A duration <= 0, -0.0 or NaN counts 0; one above 2e9 (+inf included) counts 2e9.  The prefix sums are
 *   taken in 64 bits and never wrap: mel_len[b] is the exact total (up to Ts * 2e9), cum[b,i] =
 *   min(prefix_i, INT32_MAX), and mel2ph follows the exact prefixes (t < Tm <= INT32_MAX, so the
 *   saturation of cum does not change it).
 * ctts_lr_gather_fwd: out[b,t,:] = x[b, mel2ph[b,t]-1, :] or 0.      (expand + pad/crop)
 * ctts_lr_gather_bwd: dx[b,i,:] = sum over the contiguous frame run of phoneme i of dy.   */
int ctts_lr_index(const void* dur, int dur_is_float, int round_mode, const uint8_t* pad, int B, int Ts, int Tm,
                  int32_t* mel2ph, int64_t* mel_len, int32_t* cum, void* stream);
int ctts_lr_gather_fwd(const float* x, const int32_t* mel2ph, float* out, int B, int Ts, int Tm, int C, void* stream);
int ctts_lr_gather_bwd(const float* dy, const int32_t* cum, float* dx, int B, int Ts, int Tm, int C, void* stream);

/* Target-side pitch chain of the cwt pitch branch in ONE launch (csrc/pitch.hip; utils/pitch_tools.py:27-36 f0_to_coarse, :258-294 inverse_cwt_torch /
 * cwt2f0 / cwt2f0_norm with pitch_norm "log", and the denormalisation of modules.py:1071-1091): per utterance b
 *   rec[t] = sum_{j < nscale} spec[b,t,j] * (j + 3.5)^-2.5;  rec = (rec - mean_t rec) / std_t rec  (unbiased, over all T columns);
 *   f0[b,t] = log2(exp(rec * f0_std[b] * std_scale + f0_mean[b]) + eps)  (columns T .. width-1 repeat column T-1);
 *   f0_denorm = unvoiced ? 0 : 2^f0;   ids = f0_to_coarse(f0_denorm) in [1, f0_bin - 1]  (mel_min / mel_max = 1127 ln(1 + f / 700) at 50 / 1100 Hz).
 * spec [B,T,ld_spec]; unvoiced = uv[b,t] > 0 (uv float [B,width]) or, with uv NULL, spec[b,t,uv_chan] > 0 (the predictor's uv logit).
 * Outputs f0, f0_denorm [B,width] float, ids [B,width] int64.  Deterministic (ordered two-pass sums in double), no atomics, no memset. */
int ctts_cwt_pitch(const float* spec, int64_t ld_spec, int nscale, const float* f0_mean, const float* f0_std, float std_scale,
                   const float* uv, int uv_chan, float eps, float mel_min, float mel_max, int f0_bin, float* f0, float* f0_denorm,
                   int64_t* ids, int B, int T, int width, void* stream);

/* make_positions (utils/tools.py:640-652): pos = cumsum(x != 0) * (x != 0) along T.
 * src is float32 (stride `stride` elements between time steps, e.g. channel 0 of [B,T,C]) or int64 tokens. */
int ctts_positions(const void* src, int src_is_float, int64_t stride, int B, int T, int32_t* pos, void* stream);

/* ---------------------------------------------------------------------------------------
 * LayerNorm over the last dim (blocks.py:137-156 eps 1e-12; nn.LayerNorm eps 1e-5), fused with
 * inverted dropout and the non-pad row mask:  y = rowscale * drop(LN(x)).
 * planes (optional, round 6): the bf16 plane set of y in the layout of ctts_split_planes ([rows][C / 32][3][32], C % 32 == 0),
 * written by the same launch from the registers that hold y - bit-identical to ctts_split_planes(y), for the plane-kernel GEMM that
 * consumes y (FFN Conv1d, transformer_fs2.py:220-239) without a second pass over y.  The same optional argument on ctts_bn_apply (the
 * PostNet convolutions' inputs, modules.py:140-148) and ctts_bn_bwd_apply (their output gradients dZ).                               */
int ctts_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                       int rows, int C, float eps, float p_drop, const uint64_t* seed, uint32_t drop_offset,
                       const float* rowscale, uint16_t* planes, void* stream);
int ctts_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                       float* dx, float* dgamma, float* dbeta, int rows, int C, float p_drop, const uint64_t* seed,
                       uint32_t drop_offset, const float* rowscale, int accumulate, const float* dres, void* ws, float* parts,
                       void* stream);
/* accumulate != 0: dgamma / dbeta (and ctts_colsum's out) are ADDED to - gradient-accumulation fusion straight into param.grad.
 * dres (optional, [rows,C]): added to dx - the gradient arriving through the residual connection around the pre-LN sub-layer
 * (x -> LN -> f -> + x), so the autograd sum of the two paths costs no extra pass. */

/* BatchNorm1d over [rows, C] (channel-last view of nn.BatchNorm1d, modules.py:105,140-148),
 * fused with tanh (act=3) / none and inverted dropout.
 * stats: sums[0..C) = sum x, sums[C..2C) = sum x^2 (double, pre-zeroed by the call).
 * apply: y = drop(act((x-mean)*rstd*gamma+beta)).
 * bwd_reduce: sums[0..C) = sum dt, sums[C..2C) = sum dt*xhat with dt = dy*dropmask*act'(u).
 * bwd_apply: dx = gamma*rstd*(dt - sum_dt/rows - xhat*sum_dtxhat/rows); dgamma/dbeta from sums.
 *   batch_stats bit 0: train-mode statistics (the two correction terms above), bit 1: ADD to dgamma / dbeta instead of storing. */
int ctts_colstats(const float* x, double* sums, int rows, int C, void* ws, void* stream);
/* mean / rstd of the batch from ctts_colstats sums, plus the nn.BatchNorm train-mode bookkeeping (running_mean / running_var with
 * momentum and the unbiased variance, num_batches_tracked += 1; NULL pointers skip) - one launch instead of a dozen [C]-sized ops. */
int ctts_bn_finalize(const double* sums, int rows, int C, float eps, float momentum, float* mean, float* rstd, float* running_mean,
                     float* running_var, int64_t* num_batches, void* stream);
int ctts_bn_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                  float* y, int rows, int C, int act, float p_drop, const uint64_t* seed, uint32_t drop_offset,
                  uint16_t* planes /* optional plane set of y, see ctts_layernorm_fwd */, void* stream);
int ctts_bn_bwd_reduce(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                       const float* beta, double* sums, int rows, int C, int act, float p_drop, const uint64_t* seed,
                       uint32_t drop_offset, void* ws, void* stream);
int ctts_bn_bwd_apply(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, const double* sums, float* dx, float* dgamma, float* dbeta, int rows, int C,
                      int act, float p_drop, const uint64_t* seed, uint32_t drop_offset, int batch_stats,
                      uint16_t* planes /* optional plane set of dx */, void* stream);

/* Masked row softmax for attention scores S[nbatch, T, T] (in place), keys >= lens[z/nb1] get 0
 * and query rows >= len are left untouched (F.multi_head_attention_forward key_padding_mask).
 * bwd: dS = P * (dP - sum_k dP*P), in place on dP.                                            */
int ctts_softmax_fwd(float* S, const int32_t* lens, int nb0, int nb1, int T, int64_t ld, void* stream);
int ctts_softmax_bwd(const float* P, float* dP, const int32_t* lens, int nb0, int nb1, int T, int64_t ld,
                     void* stream);

/* Elementwise helpers of the backward pass.
 * act_dropout_bwd: dz = dg * dropmask/(1-p) * act'(z)          (GELU/ReLU/tanh from saved pre-activation)
 * rowscale_dropout_bwd: dv = dy * rowscale[m] * dropmask/(1-p)  (output-side dropout + pad mask)
 * colsum: out[c] (+)= scale * sum_rows x[r, c]                  (bias gradients)               */
int ctts_act_dropout_bwd(const float* dg, const float* z, float* dz, int64_t rows, int C, int act, float alpha_unused,
                         float p_drop, const uint64_t* seed, uint32_t drop_offset, void* stream);
int ctts_rowscale_dropout(const float* x, float* y, int64_t rows, int C, const float* rowscale, float p_drop,
                          const uint64_t* seed, uint32_t drop_offset, void* stream);
int ctts_colsum(const float* x, float* out, int64_t rows, int C, int64_t ld, float scale, int accumulate, void* ws, float* parts, void* stream);

/* ---------------------------------------------------------------------------------------
 * Mel front end (audio/stft.py:59-88,166-185): reflect-pad, |DFT| from the [F, 2*nbins]
 * re/im GEMM result, energy = L2 norm over bins; the two GEMMs go through ctts_gemm.          */
int ctts_reflect_pad(const float* y, float* ypad, int B, int N, int pad, int64_t ld_out, void* stream);
int ctts_stft_magnitude(const float* reim, int64_t ld_reim, float* mag, int64_t ld_mag, float* energy, int64_t frames,
                        int nbins, void* stream);
int ctts_log_clamp_transpose(const float* mel_fm, float* out, int B, int F, int n_mel, float clip, void* stream);

/* ---------------------------------------------------------------------------------------
 * Conformer block pieces (model/transformers/conformer.py).
 * GLU over the channel dim (blocks.py GLU, conformer.py:458): a [rows, 2C] -> out[r,c] = a[r,c] * sigmoid(a[r,C+c]).
 * Depthwise Conv1d k (odd), 'same' padding, no bias, channel-last (conformer.py:522-560, DepthwiseConv1d):
 *   y[b,t,c] = sum_k wT[k,c] * x[b,t+k-pad,c];  flip=1 uses wT[K-1-k] (data gradient);
 *   wgrad: dw[c,k] += sum_{b,t} dy[b,t,c] * x[b,t+k-pad,c]   (dw [C,K], pre-zeroed by the call).
 * Relative-position attention scores (conformer.py:347-431, RelativeMultiHeadAttention):
 *   relpos_softmax_fwd: P = softmax_j( (S[i,j] + shift(PS)[i,j]) * scale ) over ALL keys (no mask, conformer.py:243 vs :326),
 *     shift = Transformer-XL _relative_shift (conformer.py:423-431); P overwrites S, Pd = inverted-dropout(P) (optional).
 *   relpos_softmax_bwd: dS = P * (dP - sum_j dP*P) * scale with dP = dropmask/(1-p) * dPd, in place on dPd;
 *   relshift_bwd: dPS = inverse of the shift applied to dS.                                               */
/* Operand preparation of RelativeMultiHeadAttention.forward (conformer.py:396-407) from the packed q | k | v projection [rows, 3C] in
 * one pass: qu = q + u_bias, qv = q + v_bias [rows, C], kv = k | v [rows, 2C]; and its adjoint dqkv = (dqu + dqv) | dkv (the bias
 * gradients are column sums of dqu / dqv: ctts_colsum). */
int ctts_relattn_split_fwd(const float* qkv, const float* u_bias, const float* v_bias, float* qu, float* qv, float* kv, int64_t rows,
                           int C, void* stream);
int ctts_relattn_split_bwd(const float* dqu, const float* dqv, const float* dkv, float* dqkv, int64_t rows, int C, void* stream);
int ctts_glu_fwd(const float* a, float* out, int64_t rows, int C, void* stream);
int ctts_glu_bwd(const float* a, const float* dout, float* da, int64_t rows, int C, void* stream);
int ctts_dwconv_fwd(const float* x, const float* wT, float* y, int B, int T, int C, int K, int flip, void* stream);
int ctts_dwconv_wgrad(const float* dy, const float* x, float* dw, float* partials, int B, int T, int C, int K, int accumulate,
                      void* stream);      /* accumulate != 0: dw += (gradient-accumulation fusion straight into param.grad) */
/* partials: scratch of 128 * C * 32 floats (slice sums, reduced in a fixed order - deterministic, no atomics) */
int ctts_relpos_softmax_fwd(float* S, const float* PS, float* Pd, int nbatch, int T, float scale, float p_drop,
                            const uint64_t* seed, uint32_t drop_offset, void* stream);
int ctts_relpos_softmax_bwd(const float* P, float* dPd, int nbatch, int T, float scale, float p_drop, const uint64_t* seed,
                            uint32_t drop_offset, void* stream);
int ctts_relshift_bwd(const float* dS, float* dPS, int nbatch, int T, void* stream);

/* Embedding lookup (model/transformers/blocks.py:10-15, model/modules.py:779-788,947,958).
 * fwd: out[r,:] = weight[ids[r],:] (ids int64 [n], weight [V,C], C % 4 == 0).
 * bwd: dweight[v,:] (+)= sum over r with ids[r] == v of dy[r,:], row padding_idx forced to zero (nn.Embedding(padding_idx=..));
 *      one wave per (vocabulary row, 64-id chunk), register partial sums + one atomicAdd per channel.  padding_idx < 0: none. */
int ctts_embedding_fwd(const int64_t* ids, const float* weight, float* out, int64_t n, int C, int V, void* stream);
int ctts_embedding_bwd(const int64_t* ids, const float* dy, float* dweight, int64_t n, int C, int V, int padding_idx, int accumulate,
                       void* ws, void* stream);

/* ---------------------------------------------------------------------------------------
 * Unsupervised duration modelling.
 * ctts_neg_sqdist: AlignmentEncoder scores out[b,t,s] = -temp * sum_c (q[b,t,c]-k[b,s,c])^2  (model/modules.py:1199-1200), channel-last.
 *   q [B,Tq,C], k [B,Tk,C], out [B,Tq,Tk]; every element of out is written.  C <= 255 (a 64-key tile of C+1 floats per key lives in
 *   LDS); a larger C is refused ("C too large for the LDS tile").
 * ctts_mas: monotonic alignment search, width 1 (model/modules.py:36-75 mas_width1/b_mas; called from :863-872).
 *   attn [B,Tq,Tk] soft attention (probabilities), in_lens/out_lens [B] valid text / mel lengths;
 *   opt [B,Tq,Tk] <- hard 0/1 alignment, dur [B,Tk] <- frames per phoneme (attn_hard.sum(2)), back [B,Tq,Tk] scratch bytes. */
int ctts_neg_sqdist(const float* q, const float* k, float* out, int B, int Tq, int Tk, int C, float temp, void* stream);
int ctts_mas(const float* attn, const int32_t* in_lens, const int32_t* out_lens, float* opt, float* dur, uint8_t* back, int B,
             int Tq, int Tk, void* stream);
/* ForwardSumLoss (model/loss.py:350-377) for the whole batch in one launch: per utterance b the CTC negative
 * log-likelihood nll[b] of the target sequence 1..K_b under log_softmax([blank_logprob, attn_logprob[b,t,0..K_b-1]]) over the
 * T_b = out_lens[b] valid frames (K_b = in_lens[b]).  The reference's loss is mean_b(nll[b] / K_b) with infinities zeroed.
 *   fwd: attn_logprob [B,Tq,Tk] -> lse [B,Tq] (row normalisers), alpha [B,Tq,2*Tk+1] (log forward variables), nll [B]
 *   bwd: grad [B,Tq,Tk] = gscale[b] * d nll[b] / d attn_logprob (zero for frames >= T_b, tokens >= K_b, or nll[b] = inf)   */
int ctts_forward_sum_fwd(const float* attn_logprob, const int32_t* in_lens, const int32_t* out_lens, float blank_logprob, float* lse,
                         float* alpha, float* nll, int B, int Tq, int Tk, void* stream);
int ctts_forward_sum_bwd(const float* attn_logprob, const int32_t* in_lens, const int32_t* out_lens, float blank_logprob,
                         const float* lse, const float* alpha, const float* nll, const float* gscale, float* grad, int B, int Tq,
                         int Tk, void* stream);

/* ---------------------------------------------------------------------------------------
 * liu2021 implicit prosody modelling (model/modules.py:332-648, model/coordconv.py:140-159).
 * ctts_im2col_3x3s2: patch matrix of Conv2d(3x3, stride (1,2), padding (1,1)) (ReferenceEncoder convs, modules.py:351-361) on
 *   channel-last x[B,T,W,C]: col[(b,t,wo)][(kh*3+kw)*C + c] = x[b, t+kh-1, 2*wo-1+kw, c] (0 outside), Wo = (W-1)/2+1, C % 4 == 0.
 *   The convolution itself is ctts_gemm(col, w[Cout][kh][kw][Cin]).  ctts_col2im_3x3s2 is the adjoint (dx from dcol).
 * ctts_gru_fwd / ctts_gru_bwd: recurrent part of `ndir` independent one-layer nn.GRU sequences per utterance (1..8: the two directions
 *   of a bidirectional GRU, or several GRUs of equal H and T sharing one launch), batch_first, zero initial state; sequence d runs
 *   t = T-1..0 iff bit d of rev_mask is set
 *   (modules.py:359-361,391 ReferenceEncoder; :618-621,637 ParallelProsodyPredictor).  gate order r|z|n,
 *   n = tanh(gi_n + r * (W_hn h + b_hn)), h' = (1-z) n + z h.  The sequence runs over all T steps (the reference never packs).
 *   gi [B,T,ndir,3H] = W_ih x + b_ih (caller's GEMM); whh [ndir,3H,H]; bhh [ndir,3H]; out [B,T,ndir,H];
 *   gates [B,T,ndir,4H] <- r|z|n|(W_hn h + b_hn) saved for backward (NULL in inference).
 *   bwd: dout [B,T,ndir,H] -> dgi, dgh [B,T,ndir,3H] (gradients w.r.t. the input / hidden pre-activations) and hprev [B,T,ndir,H]
 *   (h_{t-1}); the caller forms dW_hh = dgh^T hprev and db_hh = colsum(dgh).  H in {16,32,64,128}.
 * ctts_softmax_rect_fwd/bwd: in-place masked row softmax of S[nb,Tq,Tk]; keys >= klens[b] -> 0, query rows >= qlens[b] -> 0
 *   (PhonemeLevelProsodyEncoder attention, modules.py:443-446; STL token attention :527-529).  NULL lens = no mask. */
int ctts_im2col_3x3s2(const float* x, float* col, int B, int T, int W, int C, void* stream);
int ctts_col2im_3x3s2(const float* dcol, float* dx, int B, int T, int W, int C, void* stream);
int ctts_gru_fwd(const float* gi, const float* whh, const float* bhh, float* out, float* gates, int B, int T, int H, int ndir,
                 int rev_mask, void* stream);
int ctts_gru_bwd(const float* dout, const float* out, const float* gates, const float* whh, float* dgi, float* dgh, float* hprev,
                 int B, int T, int H, int ndir, int rev_mask, void* stream);
int ctts_softmax_rect_fwd(float* S, const int32_t* klens, const int32_t* qlens, int nb, int Tq, int Tk, void* stream);
int ctts_softmax_rect_bwd(const float* P, float* dP, const int32_t* klens, const int32_t* qlens, int nb, int Tq, int Tk,
                          void* stream);

/* ---------------------------------------------------------------------------------------
 * Mel front end in ONE call (csrc/mel.hip): TacotronSTFT.mel_spectrogram (audio/stft.py:166-185) = STFT.transform (:59-88: reflect
 * padding by n_fft/2, hann-windowed DFT, hop) -> |X| -> mel filterbank -> log(clamp(., clip)) (audio_processing.py:85-91), and
 * energy = ||X||_2 per frame.  Computed as a 1024-point REAL FFT per frame (512-point complex radix-8 Stockham + even/odd split)
 * instead of the reference's 1026 x 1024 basis convolution, the filterbank as a banded GEMM on the fp32 MFMA.
 *   y [B,N] waveform in [-1,1]; window [n_fft] = analysis window zero-padded to n_fft (periodic hann); mel [B,n_mel,F],
 *   energy [B,F], F = 1 + N / hop; mag: optional [B*F, ld_mag >= 513] magnitudes (NULL = not stored).
 *   workspace: ctts_mel_spectrogram_workspace_bytes() bytes, filled once per filterbank by ctts_mel_prepare(mel_basis [n_mel,513]).
 *   Built for n_fft = 1024 (the reference's filter_length) and n_mel <= 96. */
size_t ctts_mel_spectrogram_workspace_bytes(int n_fft, int n_mel);
int ctts_mel_prepare(const float* mel_basis, int n_fft, int n_mel, float* workspace, void* stream);
int ctts_mel_spectrogram(const float* y, const int32_t* lens, const float* window, const float* workspace, float* mel, float* energy, float* mag,
                         int64_t ld_mag, int B, int N, int n_fft, int hop, int n_mel, float clip, int kmax, uint32_t* range_flag,
                         void* stream);
/* range_flag (optional, one uint32 in device OR pinned host memory, zero-initialised by the caller): the kernel stores the float bits of an
 * offending |sample| (> 1.0, or a NaN pattern) there when the waveform leaves [-1, 1] - the reference's two range asserts
 * (audio/stft.py:177-178) without a reduction pass and without a host synchronisation; valid input writes nothing. */
/* lens (optional, [B] int32): ragged batch for preprocessing (preprocessor.py:387,467 extracts one utterance at a time) - row b holds
 * lens[b] <= N samples (rest padding); reflection happens at the utterance's own end and its 1 + lens[b]/hop leading frames equal the
 * single-utterance result; the remaining frames of the row are don't-care. */
/* kmax: 1 + the highest DFT bin with a non-zero filter weight (372 for fmax 8 kHz at 22.05 kHz), or 0 = unknown (all 513 bins are kept
 * in the on-chip magnitude tile).  A smaller tile lets three workgroups share a CU instead of two; results do not depend on it as long as
 * no filter reaches beyond bin kmax-1.
 * The contract cannot be broken silently: ctts_mel_prepare records, per tile of 16 filters, the bin range that carries weight, and the
 * kernel bounds every tile's range by the row stride it was launched with.  A tile that reaches beyond kmax (a kmax that belongs to
 * another filterbank than the workspace) is not summed: its outputs are NaN for every frame, and range_flag, where given, receives
 * CTTS_MEL_FLAG_KMAX.  kmax = 0 is always safe.
 * The range check covers every sample of the waveform (of lens[b] samples for a ragged row): samples that no frame loads, which exist for
 * hop > n_fft/2 + 1, are read for the check alone. */
#define CTTS_MEL_FLAG_KMAX 0x7FC0004Bu

/* ---------------------------------------------------------------------------------------
 * Fused multi-head attention (csrc/attn.hip): exact-fp32 MFMA, flash-style - the [T,T] score / probability tensors never reach HBM in
 * the forward pass, the backward recomputes them.  d_head = C / H must be 32, 64 or 128 (ctts_mha_supported).
 *
 * ctts_mha_fwd / ctts_mha_bwd: the core of F.multi_head_attention_forward as transformer_fs2.py:385-394 calls it (q scaled by `scale` =
 *   d_head^-0.5, key-padding mask from valid lengths, no biases, no attention dropout) on the packed projection qkv [B,T,3C] (q | k | v).
 *   lens[b] (or NULL = T): keys >= lens[b] are masked, query rows >= lens[b] are ZERO rows of `out` [B,T,C].
 *   lse [B,H,T]: log2-domain log-sum-exp of the scaled scores (kept for the backward).
 *   bwd: out/dout [B,T,C]; Dws [B,H,T] and dS [B,H,T,T] are caller-provided scratch; dqkv [B,T,3C] receives all three gradients
 *   (zero at padded rows).  q_split >= 1 splits the query loop of a key tile over several waves - use 2 when B*H*T/32 waves do not fill
 *   the chip; each split writes its partial dK | dV into kv_part [q_split, B, T, 2C] (scratch, may be NULL for q_split 1) and a
 *   fixed-order sum produces the result: deterministic, no atomics.
 * ctts_relmha_fwd / ctts_relmha_bwd: the core of RelativeMultiHeadAttention (conformer.py:396-421) on channel-last projections:
 *   qu = q + u_bias, qv = q + v_bias [B,T,C]; kv [B,T,2C] (k | v); pos [T,C] = pos_proj(sinusoid rows) shared by the batch;
 *   score = (qu k^T + shift(qv pos^T)) * scale, softmax over ALL keys (the reference passes no mask, conformer.py:243),
 *   dropout(p_drop) on the probabilities (counter RNG: seed, drop_offset as in ctts_gemm), context = P v.  shift() is the
 *   Transformer-XL memory reinterpretation of conformer.py:423-431; the kernels evaluate it in closed form (no [B,H,T,T] score
 *   tensor exists, nothing but out and lse [B,H,T] has to be kept for the backward).
 *   bwd: Dws [B,H,T] and dS (ctts_relmha_workspace_floats(B,T,H) = B*H*T*(T+1) floats: d loss / d score in the layout of the
 *   reference's `padded` tensor, so that the gradient of the unshifted scores is a view of the same memory) are scratch; outputs
 *   dqu, dqv [B,T,C], dkv [B,T,2C] and dpos_b [B,T,C] = per-utterance gradient of pos (the caller sums it over B). */
int ctts_mha_supported(int C, int H);
int ctts_mha_fwd(const float* qkv, const int32_t* lens, float* out, float* lse, int B, int T, int H, int C, float scale, void* stream);
int ctts_mha_bwd(const float* qkv, const int32_t* lens, const float* out, const float* dout, const float* lse, float* Dws, float* dS,
                 float* kv_part, float* dqkv, int B, int T, int H, int C, float scale, int q_split, void* ws, void* stream);
/* ws: the per-stream workspace (ctts_workspace_bytes()) - the dQ = dS K reduction is split in two when the launch would not fill the
 * chip, and the pieces are summed through it in a fixed order; NULL = never split. */
size_t ctts_relmha_workspace_floats(int B, int T, int H);
int ctts_relmha_fwd(const float* qu, const float* qv, const float* kv, const float* pos, float* out, float* lse, int B, int T,
                    int H, int C, float scale, float p_drop, const uint64_t* seed, uint32_t drop_offset, void* stream);
int ctts_relmha_bwd(const float* qu, const float* qv, const float* kv, const float* pos, const float* out,
                    const float* dout, const float* lse, float* Dws, float* dS, float* dqu, float* dqv, float* dkv,
                    float* dpos_b, int B, int T, int H, int C, float scale, float p_drop, const uint64_t* seed, uint32_t drop_offset,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * Variance / duration terms of CompTransTTSLoss (model/loss.py:123-243) as one kernel pair (csrc/loss.hip):
 *   terms[8] = {pdur, wdur, sdur, C, uv, f0_mean, f0_std, energy}, each already multiplied by its lambda (lambdas5 = {lambda_ph_dur,
 *   lambda_word_dur, lambda_sent_dur, lambda_f0, lambda_uv}; lambda_word / lambda_sent <= 0 switch the term off as the reference does).
 *   log_d, e_pred, e_tgt [B,Ts] float; dur [B,Ts] int64 (dur_is_float 0) or float32 (1, the MAS durations of learn_alignment);
 *   texts [B,Ts] int64 and sil_ids3 = the three silence token ids that delimit words (loss.py:30-33); src_pad / mel_pad uint8, 1 = pad;
 *   cwt [B,Tm,11] (10 cwt bins + uv logit), cwt_spec [B,Tm,10], uv [B,Tm]; f0 statistics [B]; cwt_l2: 0 = l1, 1 = mse.
 *   Scratch kept for the backward: partials [B,16], wsum [B,2,Ts+1], denoms [4].  Deterministic (no atomics, no memset nodes:
 *   torch's multi-block reduction mis-replays its semaphore memset inside a hipGraph on this stack).
 *   bwd: g8 = upstream gradient of every term; writes d_log_d, d_e [B,Ts], d_cwt [B,Tm,11], d_f0m, d_f0s [B].
 *   Boundaries follow torch's autograd: the linear duration clamp(exp(log_d) - 1, min 0) passes its gradient AT the bound
 *   (exp(log_d) - 1 >= 0, so log_d == 0 - every padded token of the model - has slope 1 in the word and sentence terms), |x| has
 *   slope 0 at x == 0 (cwt l1, f0 statistics, energy).  A batch without any counted word (no silence token, or no word with a positive
 *   target) gives wdur = 0/0 = NaN, as the reference does; its backward then adds NO word-term contribution (no token belongs to a
 *   counted word), so all five gradients stay finite and equal those of lambda_word = 0 - without a silence token that is also
 *   what autograd gives; with silences but only zero-target words autograd would hand NaN to those words' tokens, here the NaN value
 *   is the signal.
 * ctts_bin_loss_*: BinLoss (loss.py:380-386) = -sum(log(clamp(soft,1e-12)) * hard) / sum(hard) over n elements; partials [1024],
 *   out2 = {loss, sum hard}.  The bound is the float32 nearest to 1e-12; bwd passes the gradient at soft >= bound (the bound included,
 *   as torch's clamp) and writes 0 below it. */
int ctts_var_loss_fwd(const float* log_d, const void* dur, int dur_is_float, const int64_t* texts, const uint8_t* src_pad, const float* cwt,
                      const float* cwt_spec, const float* uv, const uint8_t* mel_pad, const float* f0m_p, const float* f0m_t,
                      const float* f0s_p, const float* f0s_t, const float* e_pred, const float* e_tgt, int B, int Ts, int Tm,
                      const float* lambdas5, int cwt_l2, const int64_t* sil_ids3, float* partials, float* wsum, float* terms, float* denoms,
                      void* stream);
int ctts_var_loss_bwd(const float* log_d, const void* dur, int dur_is_float, const int64_t* texts, const uint8_t* src_pad, const float* cwt,
                      const float* cwt_spec, const float* uv, const uint8_t* mel_pad, const float* f0m_p, const float* f0m_t,
                      const float* f0s_p, const float* f0s_t, const float* e_pred, const float* e_tgt, int B, int Ts, int Tm,
                      const float* lambdas5, int cwt_l2, const int64_t* sil_ids3, const float* partials, const float* wsum,
                      const float* denoms, const float* g8, float* d_log_d, float* d_cwt, float* d_f0m, float* d_f0s, float* d_e,
                      void* stream);
int ctts_bin_loss_fwd(const float* soft, const float* hard, int64_t n, float* partials, float* out2, void* stream);
int ctts_bin_loss_bwd(const float* soft, const float* hard, const float* out2, const float* g, float* dsoft, int64_t n, void* stream);
/* ctts_masked_loss_*: sum_i w_i l(pred_i, target_i) / sum_i w_i over n elements, l = |p-t| (kind 0), (p-t)^2 (1) or BCE-with-logits (2):
 *   the f0 / uv terms of pitch_type "frame" and "ph" (loss.py:173-178,206-219) and the frame-level energy term (loss.py:238-242).
 *   partials [1024], out2 = {loss, sum w}; bwd writes dpred [n] = g * w_i * l'(p_i, t_i) / sum w.  Ordered two-stage reduction. */
int ctts_masked_loss_fwd(const float* pred, const float* target, const float* weight, int64_t n, int kind, float* partials, float* out2,
                         void* stream);
int ctts_masked_loss_bwd(const float* pred, const float* target, const float* weight, const float* out2, const float* g, float* dpred,
                         int64_t n, int kind, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused gradient clipping + Adam over flat fp32 arenas (train.py:118-125, model/optimizer.py:22-53):
 *   total = ||g||_2 ; g <- g * min(1, max_norm / (total + 1e-6))  (nn.utils.clip_grad_norm_; max_norm <= 0: no clipping)
 *   g <- g + weight_decay * p ; m <- b1 m + (1-b1) g ; v <- b2 v + (1-b2) g^2
 *   p <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)           (torch.optim.Adam, amsgrad off)
 * p, g, m, v: n floats each, 16-byte aligned.  lr: device scalar.  state: CTTS_ADAM_STATE_FLOATS device floats {sum of squares of this
 * call (output), step count t-1 (incremented here), total norm of this call (output), CTTS_ADAM_PARTIALS per-block partial sums
 * (scratch)} - all device resident so that the launches replay inside a hipGraph.  The norm is reduced in a FIXED order (no atomics):
 * data-parallel replicas with bit-identical gradients stay bit-identical.  state[2] reports the norm also when max_norm <= 0.
 * Non-finite gradients: with max_norm > 0 a NaN norm gives a NaN clip coefficient (min(1, NaN) = NaN, as clip_grad_norm_'s clamp), so
 * EVERY element of p, m and v becomes NaN - a poisoned step is visible, never a silently unclipped one.  With max_norm <= 0 nothing
 * couples the elements and only those whose own gradient is NaN are lost.  n == 0 returns at once and leaves state untouched. */
#define CTTS_ADAM_PARTIALS 2048
#define CTTS_ADAM_STATE_FLOATS (3 + CTTS_ADAM_PARTIALS)
int ctts_adam_clip_step(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, float beta1, float beta2, float eps,
                        float weight_decay, float max_norm, float* state, void* stream);

/* Masked L1 of the two mel predictions in one pass (CompTransTTSLoss mel / postnet-mel terms, model/loss.py:130-138,
 * 303-304): rows with pad[row] != 0 count as zeros, w[row] = (sum_c |target[row,c]| != 0),
 *   sums = { sum w |p1 - t|, sum w |p2 - t|, sum w }  ->  loss_k = sums[k] / (C * sums[2]);   roww [rows] <- w (kept for backward);
 *   sums need NOT be initialised: its three floats are written, never accumulated into (rows == 0 writes three zeros).
 *   ws: the stream's workspace (ordered multi-workgroup sum, same bits on every call) or NULL (one workgroup does all rows).
 * bwd: d1, d2 = g[k] * sign(p_k - t) * w / (C * sums[2]) with g the two upstream scalars (device). */
int ctts_mel_l1_fwd(const float* p1, const float* p2, const float* tgt, const uint8_t* pad, float* sums, float* roww, int64_t rows,
                    int C, void* ws, void* stream);
int ctts_mel_l1_bwd(const float* p1, const float* p2, const float* tgt, const float* roww, const float* sums, const float* g, float* d1,
                    float* d2, int64_t rows, int C, void* stream);

/* ---------------------------------------------------------------------------------------
 * HiFi-GAN V1 vocoder, inference (csrc/vocoder.hip; comprehensive-transformer-tts_amd/vocoder.py).  Replaces hifigan/models.py:112-173
 * `Generator.forward` as called by utils/model.py:74-92 `vocoder_infer` (synthesize.py:196, utils/tools.py:206-350).
 * ctts_vocoder_conv: one Conv1d of the generator per launch, implicit GEMM on the MFMA, input tile + halo staged once per 32 channels.
 *   transposed_u == 0: Conv1d(Cin, Cout, k, stride 1, dilation dil, padding dil (k - 1) / 2), k odd  - conv_pre (models.py:117),
 *     ResBlock convs1 / convs2 (models.py:24-86); T_out = T.
 *   transposed_u == u >= 1: ConvTranspose1d(Cin, Cout, k, stride u, padding (k - u) / 2), k % u == 0, (k - u) even - ups (models.py:
 *     121-131), run as the polyphase k/u-tap GEMM with N = u Cout; T_out = T u.
 *   x: element (b, t, c) at x[b sxb + t sxt + c sxc] (any strides: the mel's [B, 80, T] view of a [B, T, 80] tensor is sxc = 1);
 *   act_in = 1 applies leaky_relu(., slope) to x on load (models.py:98,100,150).
 *   w: packed weight [roundup(N, 128)][taps][roundup(Cin, 32)] fp32, zero padded (N = Cout or u Cout; taps = k or k / u):
 *     Conv1d          w[co][tap][ci]         = weight[co][ci][tap]
 *     ConvTranspose1d w[r Cout + co][tap][ci] = weight[ci][co][r + (k / u - 1 - tap) u]
 *     16-byte aligned.  w_planes: ctts_split_planes of w (ld = taps roundup(Cin, 32)), required when bf16_split != 0.
 *   out [B, T_out, Cout] dense: out = beta * out + alpha * (conv + bias[co] + R[b, t, co]); bias / R may be NULL; beta == 0 never
 *     reads out.  out must not alias x.
 *   bf16_split != 0: the exact three-way bf16 split of include/ctts.h's plane kernels (six MFMA terms, fp32 accumulation, products
 *     within one fp32 rounding); 0: exact fp32 MFMA.  Bit-reproducible (no atomics).
 * ctts_vocoder_post: out[b, t] = tanh(bias[0] + sum_{tap < k, c} leaky_relu(x[b, t + tap - (k - 1) / 2, c], slope) w[tap][c]),
 *   x [B, T, C] dense, out [B, 1, T] - conv_post with its leaky_relu (default slope 0.01) and tanh (models.py:161-163); fp32 VALU.
 * Length-aware (ragged) batches: `lens` (device int32 [B], one mel-frame count per utterance; NULL = dense, every utterance T rows)
 *   and `len_mul` >= 1 (the layer's input rows per mel frame: 1 up to the first upsampler, then the running product of the rates).
 *   Utterance b's input then has Tb = min(max(lens[b], 0) len_mul, T) rows and the layer computes exactly what a B = 1 call on
 *   x[b, :Tb] computes, bit for bit: rows at or beyond Tb read as zero for every tap, R and `beta * out` are read for valid output
 *   rows only, the transposed conv's row range and phase scatter end at Tb (its first row does not depend on the length, so the
 *   128-row tiles stay anchored at row 0 of each utterance).  Output rows at or beyond Tb (Tb u) are NOT written by ctts_vocoder_conv
 *   (nothing reads them); ctts_vocoder_post_ragged writes exact zeros there.  The content of x[b, Tb:] is never read (NaN / Inf there
 *   is harmless), lens[b] > T / len_mul behaves as T (clamped in the kernel), lens[b] <= 0 is an empty utterance: nothing is written
 *   by the conv, an all-zero row by the post kernel (our own definition: the reference raises for an empty mel).  The launch grid is
 *   sized by the padded T (no host read of lens, no sync; a tile at or beyond its utterance's end returns before it stages anything),
 *   so a captured graph may be replayed with other values in the same lens buffer.  Still one launch per layer and no atomics.
 * Descriptors must be zero-initialised (fields added later default to 0). */
typedef struct ctts_vconv_desc {
  const float* x;
  int64_t sxb, sxt, sxc;
  int32_t B, T, Cin, Cout, k, dil;
  int32_t transposed_u;
  int32_t act_in; float slope;
  const float* w; const uint16_t* w_planes;
  const float* bias;
  const float* R;
  float* out;
  float alpha, beta;
  int32_t bf16_split;
  const int32_t* lens; int32_t len_mul;
} ctts_vconv_desc;
int ctts_vocoder_conv(const ctts_vconv_desc* d, void* stream);
int ctts_vocoder_post(const float* x, int B, int T, int C, int k, const float* w, const float* bias, float slope, float* out,
                      void* stream);
int ctts_vocoder_post_ragged(const float* x, int B, int T, int C, int k, const float* w, const float* bias, float slope, float* out,
                             const int32_t* lens, int len_mul, void* stream);

/* ---------------------------------------------------------------------------------------
 * MelGAN vocoder, inference (comprehensive-transformer-tts_amd/melgan.py; the generator of descriptinc/melgan-neurips
 * mel2wav/modules.py, which utils/model.py:42-92 fetches through torch.hub for `vocoder.model: "MelGAN"`).  It runs on
 * ctts_vocoder_conv_melgan - ctts_vocoder_conv's kernels, layer description (`conv`), arithmetic and ragged contract, with two
 * extensions that ride behind it in a descriptor of their own (ctts_vconv_desc keeps its layout: the ABI version does not move) - and
 * on a reflecting conv_post.  All fields 0 / NULL: exactly ctts_vocoder_conv(&conv).
 *   pad_mode = 1 (transposed_u == 0 only): the Conv1d is preceded by ReflectionPad1d(dil (k - 1) / 2) instead of zero padding: input
 *     row ti outside [0, Tb) is read at -ti or 2 (Tb - 1) - ti, where Tb is the utterance's OWN row count (T, or the ragged
 *     min(lens[b] len_mul, T)), so utterance b is still computed bit for bit as its B = 1 call and rows at or beyond Tb are never
 *     read.  DOMAIN: Tb > dil (k - 1) / 2, as for torch's ReflectionPad1d; a dense T at or below the padding is rejected, a shorter
 *     device-given length has its reflected rows clamped into [0, Tb) - memory-safe, not a reflection.
 *   x2 != NULL (k == 1, transposed_u == 0 only): a 1x1 conv of TWO inputs, out = W [act(x) ; x2] (+ bias, R, alpha / beta as above):
 *     the K loop runs over the 32-channel chunks of x (activated as act_in says), then over those of x2 [B, T, Cin2] (element
 *     (b, t, c) at x2[b sx2b + t sx2t + c], never activated); w is [roundup(Cout, 128)][1][roundup(Cin, 32) + roundup(Cin2, 32)],
 *     x's columns first.  One GEMM of K = Cin + Cin2 for the ResnetBlock's `shortcut(x) + block(x)`: W = [W_block.4 | W_shortcut],
 *     bias = their sum.  out must alias neither input.  conv.w_planes: the split of that whole matrix.
 *   ctts_vocoder_post_reflect: ctts_vocoder_post / _post_ragged (lens may be NULL: dense) with ReflectionPad1d((k - 1) / 2) in
 *     front of the conv, reflecting at the utterance's own end; exact zeros from row Tb on.  Same domain as pad_mode = 1.
 *   Arithmetic, ragged contract and bit-reproducibility are those of the HiFi-GAN block above. */
typedef struct ctts_vconv_melgan_desc {
  ctts_vconv_desc conv;
  int32_t pad_mode;
  const float* x2; int64_t sx2b, sx2t; int32_t Cin2;
} ctts_vconv_melgan_desc;
int ctts_vocoder_conv_melgan(const ctts_vconv_melgan_desc* d, void* stream);
int ctts_vocoder_post_reflect(const float* x, int B, int T, int C, int k, const float* w, const float* bias, float slope, float* out,
                              const int32_t* lens, int len_mul, void* stream);

/* ---------------------------------------------------------------------------------------
 * HiFi-GAN vocoder, fp16 mode (csrc/vocoder_h.hip; vocoder.Generator called as g(mel, lens, precision="fp16")).  The same layers, shapes,
 * weight layout (ConvTranspose1d polyphase form included), epilogue and ragged contract as ctts_vocoder_conv / ctts_vocoder_post above;
 * what differs is the number format.  The fp32 entry points and ctts_vconv_desc are untouched by it.  Arithmetic contract:
 *   weights     folded in fp32 as for the fp32 mode, then rounded ONCE to fp16 (round to nearest even; a value beyond +-65504 is
 *               saturated to it) and packed [roundup(N, 128)][taps][roundup(Cin, 32)] fp16, zero padded, 16-byte aligned.  Biases stay fp32.
 *   input       x_f32 = 1: fp32 elements read through (sxb, sxt, sxc) - the mel, whose transposed [B, T, 80] view needs no copy - and
 *               rounded to fp16 when staged; x_f32 = 0: fp16 elements (strides in elements; dense [B, T, C] rows are read 16 bytes at a time).
 *   activations every inter-layer tensor is fp16 [B, T, C] dense, the ResBlocks' `xs` accumulator included (nothing is kept in fp32).
 *   operand     fp16(leaky_relu(float(x), slope)): computed in fp32, rounded once (act_in = 0: fp16(float(x))).
 *               Saturation to +-65504 belongs to a rounding: an fp16 input that is read without one (act_in = 0, dense rows) reaches the
 *               MFMA as it is, an inf included.  The generator never does this: every fp16-input layer has act_in = 1 and no stored
 *               activation is inf.
 *   products    v_mfma_f32_32x32x16_f16, fp32 accumulation over the whole K = taps x Cin in a fixed order (32-channel chunk, then tap,
 *               then channel); no atomics, every output element is one lane's accumulator: bit-reproducible run to run, and independent
 *               of the tile shape the launcher picks (256-row tiles for large layers, 128-row tiles otherwise).
 *   epilogue    fp32: v = beta * float(out) + alpha * (acc + bias[co] + float(R)), R and out read from fp16 (beta == 0 never reads out),
 *               then ONE rounding to fp16 on store, round to nearest even, saturated to +-65504: no inf is ever produced (NaN stays NaN).
 *   conv_post   ctts_vocoder_post_h reads fp16, computes leaky_relu, the 7-tap dot product (fp32 weights) and tanh on the VALU in fp32,
 *               writes fp32 [B, 1, T].  lens == NULL: dense; otherwise the ragged form (exact zeros from row Tb on).
 *   subnormals  fp16 subnormal operands are NOT flushed by v_mfma_f32_32x32x16_f16 on gfx950 and subnormal results are stored as such
 *               (the kernels run with the default fp16 denormal mode): tests/test_vocoder_half_gpu.py::test_conv_subnormal_operands
 *               multiplies subnormal weights by subnormal-free and subnormal inputs and gets the exact products.  No per-layer scale
 *               is applied.
 * Ragged batches: lens / len_mul exactly as above - tiles anchored at row 0 of each utterance, the utterance's own length in T's place
 *   everywhere, tiles beyond its end return before they stage anything, lens[b] > T behaves as T, the content of x[b, Tb:] is never read,
 *   no host read of lens.  Descriptors must be zero-initialised. */
typedef struct ctts_vconv_h_desc {
  const void* x;
  int64_t sxb, sxt, sxc;
  int32_t x_f32;
  int32_t B, T, Cin, Cout, k, dil;
  int32_t transposed_u;
  int32_t act_in; float slope;
  const uint16_t* w;
  const float* bias;
  const uint16_t* R;
  uint16_t* out;
  float alpha, beta;
  const int32_t* lens; int32_t len_mul;
} ctts_vconv_h_desc;
int ctts_vocoder_conv_h(const ctts_vconv_h_desc* d, void* stream);
int ctts_vocoder_post_h(const uint16_t* x, int B, int T, int C, int k, const float* w, const float* bias, float slope, float* out,
                        const int32_t* lens, int len_mul, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fastformer additive attention (block_type "fastformer"; reference model/transformers/fastformer.py FastAttention).  Rows (b, t) run
 * over the PADDED length T (B*T rows), columns c = h*D + j for H heads of size D (C = H*D, D a power of two <= 64, C % 64 == 0,
 * C <= 1024).  Logits s [B*T, H] (row stride lds) come from the logit projections; lens int32 [B] are the valid lengths.
 *   z[b,t,h] = s / div + (t < lens[b] ? -10000 : 0)          (div = sqrt(D); fp32, in this order: the reference's inverted mask)
 *   ctts_fastformer_pool_fwd   alpha = softmax_t(z) per (b, h);  p[b, c] = sum_t alpha[b,t,h] V[b,t,c];  stats [B, H, 2] = (max, denominator)
 *                              for the backward.  ws: ctts_fastformer_workspace_floats(B, T, H, C) floats (per-chunk partials).
 *   ctts_fastformer_pool_bwd   dV = dV_in (NULL = 0) + alpha dp[b];  ds = alpha (sum_j V dp - sum_j p dp) / div   (dV, ds dense; dV may be dV_in)
 *   ctts_fastformer_bcast      Y[b,t,:] = X[b,t,:] * p[b,:]    (Y dense [B*T, C])
 *   ctts_fastformer_bcast_bwd  dy = dY1 + dY2 (NULL = 0);  dX = dX_in (NULL = 0) + dy p[b];  dp[b, c] = sum_t dy X   (dX may be dX_in)
 *   ctts_fastformer_resdrop    backward = 0: y = rowscale * (x + dropout(t));  backward = 1 (x unused): y = rowscale * dropout(t) and
 *                              y2 = rowscale * t, with t the incoming gradient.  rowscale [rows] or NULL; the dropout mask is the one of
 *                              the GEMM epilogues (seed, drop_offset, index row * C + col).
 * Reductions over T are per 32-row chunk and combined in chunk order: no atomics, bit-reproducible.  All stream-ordered, capturable. */
size_t ctts_fastformer_workspace_floats(int B, int T, int H, int C);
int ctts_fastformer_pool_fwd(const float* s, int64_t lds, const float* V, int64_t ldv, const int32_t* lens, float* p, float* stats,
                             float* ws, int B, int T, int H, int C, float div, void* stream);
int ctts_fastformer_pool_bwd(const float* dp, const float* p, const float* stats, const float* s, int64_t lds, const float* V,
                             int64_t ldv, const int32_t* lens, const float* dV_in, float* dV, float* ds, int B, int T, int H, int C,
                             float div, void* stream);
int ctts_fastformer_bcast(const float* X, int64_t ldx, const float* p, float* Y, int B, int T, int C, void* stream);
int ctts_fastformer_bcast_bwd(const float* dY1, const float* dY2, const float* X, int64_t ldx, const float* p, const float* dX_in,
                              float* dX, float* dp, float* ws, int B, int T, int C, void* stream);
int ctts_fastformer_resdrop(const float* x, const float* t, float* y, float* y2, int64_t rows, int C, const float* rowscale,
                            float p_drop, const uint64_t* seed, uint32_t drop_offset, int backward, void* stream);

/* ---------------------------------------------------------------------------------------
 * Griffin-Lim vocoder (csrc/griffinlim.hip): audio/stft.py:22-134 STFT.transform / inverse and audio/audio_processing.py:66-82
 * griffin_lim on a 1024-point real FFT per frame (one wave per frame, no dense basis).  Built for n_fft = 1024, hop = 256 only (other
 * sizes return an error); the analysis / synthesis window is the [1024] table handed to the prepare call (periodic hann zero-padded to
 * n_fft in the product).  Every entry point is stream-ordered, allocation-free, atomic-free (bit-reproducible) and capturable.
 *   workspace  griffinlim_workspace_bytes() bytes: twiddles, window, window^2; filled once by griffinlim_prepare(window [1024]).
 *   transform  x [B,N] (N > 512) -> mag, phase: element (b, k, f) at b sb + k sk + f sf, k < 513, F = 1 + N / 256.  lens (device int32
 *              [B] or NULL): samples per utterance; each reflects at its own end, frames past 1 + lens[b] / 256 are written as 0.
 *   istft_frames   (mag, phase) (same strides) -> Y [B][F][1024], the windowed inverse-DFT frames before overlap-add; magT (optional,
 *              [B][F][513]) receives a frame-major copy of mag, the operand of griffinlim_iter.
 *   griffinlim_iter  Y_in -> Y_out (distinct buffers): overlap-add of Y_in, transform with reflect padding, magnitude replaced by magT
 *              (phase kept; (mag, 0) where |X| = 0), inverse - one Griffin-Lim iteration.
 *   griffinlim_iter_momentum  the same launch as one iteration of fast Griffin-Lim (Perraudin et al. 2013, the momentum of librosa /
 *              torchaudio): with X the rebuilt spectrum, A = X - coef T_prev, T_prev <- X, and A is rescaled to magT by the rule above
 *              (m A / |A|, (m, 0) where |A| = 0; not librosa's + 1e-16).  coef = momentum / (1 + momentum), in [0, 1).  state
 *              (griffinlim_state_floats(B, F) floats, one slot per frame, layout private to the library) holds T_prev; a slot is read
 *              and rewritten in place by the one wave that owns the frame.  first != 0: the state counts as zero and is only written
 *              (it need not be initialised, NaN included).  coef = 0 gives griffinlim_iter's bits.
 *   istft_frames_seeded  istft_frames with the phase drawn on the device instead of read: theta(b, k, f) = 2 pi u, u in [0, 1) a
 *              counter-based hash (the dropout kernels' ctts_mix32) of (*seed, b, k, f) alone - not of B, F or frames.  seed is a
 *              DEVICE int64, read by the kernel: a captured graph replays with whatever it holds then.
 *   istft_ola  Y -> out [B, ld_out >= 256 (F - 1)]: overlap-add in ascending frame order, / window_sumsquare where > FLT_MIN, * 4, crop
 *              512 at both ends; samples past 256 (frames[b] - 1) are written as 0.
 * frames (device int32 [B] or NULL = F): frames per utterance of a ragged batch.  istft_frames(_seeded) / istft_ola need F >= 2 and clamp
 *   frames[b] to [2, F]; griffinlim_iter(_momentum) needs F >= 4 and clamps to [4, F] (its transform needs more than n_fft/2 samples). */
size_t ctts_griffinlim_workspace_bytes(int n_fft, int hop);
int ctts_griffinlim_prepare(const float* window, int n_fft, int hop, float* workspace, void* stream);
int ctts_stft_transform(const float* x, const int32_t* lens, const float* workspace, float* mag, float* phase, int64_t sb, int64_t sk,
                        int64_t sf, int B, int N, int n_fft, int hop, void* stream);
int ctts_istft_frames(const float* mag, const float* phase, int64_t sb, int64_t sk, int64_t sf, const int32_t* frames,
                      const float* workspace, float* Y, float* magT, int B, int F, int n_fft, int hop, void* stream);
int ctts_griffinlim_iter(const float* Y_in, const float* magT, const int32_t* frames, const float* workspace, float* Y_out, int B, int F,
                         int n_fft, int hop, void* stream);
int ctts_istft_ola(const float* Y, const int32_t* frames, const float* workspace, float* out, int64_t ld_out, int B, int F, int n_fft,
                   int hop, void* stream);
size_t ctts_griffinlim_state_floats(int B, int F);
int ctts_griffinlim_iter_momentum(const float* Y_in, const float* magT, float* state, const int32_t* frames, const float* workspace,
                                  float* Y_out, float coef, int first, int B, int F, int n_fft, int hop, void* stream);
int ctts_istft_frames_seeded(const float* mag, int64_t sb, int64_t sk, int64_t sf, const int32_t* frames, const float* workspace,
                             const int64_t* seed, float* Y, float* magT, int B, int F, int n_fft, int hop, void* stream);

/* ---------------------------------------------------------------------------------------
 * Gradient all-reduce of the data-parallel step (SURVEY.md section 8(b) `ctts_allreduce_*`, 8(e); replaces what
 * `DistributedDataParallel(model, device_ids=[rank])` does after backward in the reference: train.py:29-35,58,112).
 *   ctts_comm_unique_id  rank 0 draws CTTS_COMM_ID_BYTES opaque bytes (ncclGetUniqueId) and hands them to every rank by any side
 *                        channel (the Python host: `torch.distributed.broadcast_object_list`; a C host: its own launcher)
 *   ctts_comm_create     one communicator per process, bound to the CURRENT HIP device (ncclCommInitRank; collective: every rank calls it)
 *   ctts_allreduce_mean  buf[i] <- mean over ranks of buf[i], in place, n floats, stream-ordered on `stream` and capturable into a
 *                        hipGraph (ncclAllReduce, ncclFloat32, ncclAvg: the division by the world size rides inside the collective).
 *                        The product calls it once per gradient BUCKET (4 contiguous ranges of the flat gradient arena, one per
 *                        backward stage, 8 - 60 MB each) on a side stream while the next stage runs.
 *   ctts_comm_destroy    ncclCommDestroy
 * RCCL (librccl.so.1) is bound at run time by dlopen - libctts_hip.so does not link it, single-GPU use never loads it; when it cannot be
 * loaded these calls fail with a text, nothing else is affected.  Which collective runs where: `dp.BucketedReducer` uses
 * `torch.distributed` (backend "nccl" = the same RCCL) by default because the rendezvous, the process group and its watchdog are
 * already there under a PyTorch host; `CTTS_ABI_COLLECTIVE=1` (or `BucketedReducer(..., abi_collective=True)`) routes the bucket
 * all-reduces through these entry points instead - same bytes, same stream, bit-identical result (tests/test_dp_gpu.py). */
#define CTTS_COMM_ID_BYTES 128
int ctts_comm_unique_id(void* id_out /* CTTS_COMM_ID_BYTES host bytes */);
int ctts_comm_create(void** comm_out, int32_t nranks, int32_t rank, const void* id /* CTTS_COMM_ID_BYTES host bytes */);
int ctts_comm_destroy(void* comm);
int ctts_allreduce_mean(float* buf, int64_t n, void* comm, void* stream);

/* ---------------------------------------------------------------------------------------
 * Pitch targets on the device (csrc/pitchtrack.hip): wav -> f0 -> the p_targets of the cwt pitch branch.
 *
 * ctts_pitch_track: a batched, length-aware F0 tracker (Boersma-style autocorrelation; a specified algorithm of this project, NOT a
 * clone of parselmouth's to_pitch_ac, which the reference calls at utils/pitch_tools.py:106-108 - no path search across frames).
 *   wav [B,N] fp32 in [-1,1]; lens [B] int32 samples per utterance (NULL = N); f0 [B,F] Hz (0 = unvoiced), strength [B,F],
 *   F = 1 + N / hop: the mel kernel's framing, frame t centred at sample t hop, samples outside [0, len) read as 0, frames at or
 *   beyond 1 + len / hop give 0.  Per frame: 1024 samples, minus their mean, times the periodic hann window; 2048-point zero-padded
 *   power spectrum and back = autocorrelation r; rn(tau) = (r(tau) / r(0)) / (r_w(tau) / r_w(0)) with the window's own
 *   autocorrelation r_w (workspace); candidates = local maxima (rn(tau) > rn(tau-1) and rn(tau) >= rn(tau+1)) over the integer lags
 *   [floor(sr / f0_max), ceil(sr / f0_min)], lag and height refined by a parabola through the three points; the winner maximises
 *   height - 0.01 log2(f0_min tau / sr) (ties: the smaller lag); voiced when its height >= voicing_threshold and the frame's peak |x|
 *   >= silence_threshold * the utterance's peak |x| over [0, len).  r(0) <= 0 or non-finite (digital silence, NaN input) and frames
 *   without a candidate give f0 = strength = 0; an unvoiced frame with a candidate keeps its strength.
 *   DOMAIN: hop >= 1, 0 < f0_min < f0_max, floor(sr / f0_max) >= 2 and ceil(sr / f0_min) + 1 < 512 (the lags, with one neighbour
 *   on each side, stay inside the first half of the 1024-sample frame, where r_w is far from 0); anything else is refused with an
 *   error string before any launch.  peak [32 B]: scratch of the call (the utterance peaks in 32 slices each, a launch of their own).
 *   workspace: ctts_pitch_track_workspace_bytes() bytes, filled once by ctts_pitch_track_prepare (twiddles and r_w in double precision).
 *   No float atomics, no inter-workgroup waits: bit-reproducible, and an utterance's result does not depend on the batch around it.
 *
 * ctts_f0_targets: the reference's offline chain per utterance (one workgroup each): utils/pitch_tools.py:152-190 convert_continuos_f0 +
 * log (start / end located BY VALUE like :171-172), preprocessor.py:612-618 get_f0cwt (np.mean / np.std, ddof 0, over the utterance's own
 * frames), :193-209 get_lf0_cwt = real(cwt((cont_lf0 - mean) / std)) with pycwt's published definition for the Mexican hat at
 * dt = 0.005, dj = 1, s0 = 0.01, J = 9: zero-pad to M = 2^ceil(log2 n), W_j = ifft(fft(x, M) sqrt(s_j w_1 M) psi(s_j w))[:n],
 * psi(f) = f^2 exp(-f^2 / 2) / sqrt(Gamma(2.5)), s_j = s0 2^j, w = 2 pi fftfreq(M, dt).  M is the utterance's own power of two.
 *   f0 [B,F] Hz (0 = unvoiced); frames [B] int32 (clamped to [0, F]); uv [B,F] = (f0 == 0) as 0 / 1 floats (the dataset's polarity,
 *   norm_interp_f0); cont_lf0 [B,F]; mean_std [B,2]; cwt_spec [B,F,10]; valid [B] int32.  valid = 0 - and every output row of the
 *   utterance 0 - when it has no voiced frame, when its cont_lf0 is constant (std == 0, decided exactly: max == min), or when any output
 *   is not finite - which includes every utterance of two frames: at M = 2, w_1 = 2 pi fftfreq(2, dt)[1] is negative and sqrt(s_j w_1 M)
 *   is NaN.  Frames at or beyond frames[b] are 0 in every output.  DOMAIN: 1 <= F <= 4096 (refused otherwise), nscale = 10.
 * ctts_norm_interp_f0: the model-side f0 target (utils/pitch_tools.py:39-66 with pitch_norm "log", use_uv): log2(f0 + eps), 0 at
 * unvoiced frames, then np.interp over the unvoiced positions (edge values held); all unvoiced -> zeros.  Same kernel, other mode. */
size_t ctts_pitch_track_workspace_bytes(void);
int ctts_pitch_track_prepare(float* workspace, void* stream);
int ctts_pitch_track(const float* wav, const int32_t* lens, const float* workspace, float* peak, float* f0, float* strength, int B, int N,
                     int sr, int hop, float f0_min, float f0_max, float voicing_threshold, float silence_threshold, void* stream);
int ctts_f0_targets(const float* f0, const int32_t* frames, float* uv, float* cont_lf0, float* mean_std, float* cwt_spec, int32_t* valid,
                    int B, int F, void* stream);
int ctts_norm_interp_f0(const float* f0, const int32_t* frames, float* f0_norm, float* uv, int B, int F, float eps, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dataset preparation on the device (csrc/preprocess.hip): the three host steps of the reference's
 * preprocessor/preprocessor.py - silence trim (:363-368), beta-binomial alignment prior (:551-560), outlier filter and the moments of
 * the normalisation statistics (:620-628, StandardScaler.partial_fit).  fp32 data, lengths are int32 device arrays and are clamped to
 * the padded width in the kernels; stream-ordered, no allocation, no host sync, no float atomics: bit-reproducible run to run, and an
 * utterance's result does not depend on the batch around it.
 *
 * ctts_trim_silence: librosa 0.7.2 effects.trim with ref = np.max, restated (PARITY UNPINNED: librosa is not installed where this
 * project is built).  wav [B,N], lens [B] samples.  The utterance's own lens[b] samples are reflect-padded by frame_length / 2 on each
 * side; frames f = 0 .. lens[b] / hop; mse_f = mean of squares of padded samples [f hop, f hop + frame_length), accumulated in double;
 * ref = max_f mse_f; frame f is non-silent iff 10 log10(max(1e-10, mse_f)) - 10 log10(max(1e-10, ref)) > -top_db (evaluated in double);
 * start[b] = hop first, end[b] = min(lens[b], hop (last + 1)); no non-silent frame (or lens[b] <= 0) gives start = end = 0.  Digital
 * silence has mse_f = ref = 0, so every frame is 0 dB below the reference: nothing is trimmed, as in librosa.
 *   Samples at or beyond lens[b] are never read.  DOMAIN: lens[b] > frame_length / 2 (reflection); a shorter device-given length has
 *   its reflected indices clamped into [0, lens[b]) - memory-safe, not librosa's answer.  frame_length >= 2, hop >= 1, B <= 65535.
 *   workspace: ctts_trim_silence_workspace_bytes(B, N, hop) bytes; after the call it holds mse as float [B][1 + N / hop] (frames at or
 *   beyond 1 + lens[b] / hop are 0), each within one float rounding of the double evaluation.
 *
 * ctts_attn_prior: out[b][s][t] = BetaBinom.pmf(t; n = mel_lens[b], a = sf (s + 1), b = sf (src_lens[b] - s)) for s < src_lens[b] and
 * t < mel_lens[b], 0 elsewhere (the zero padding of pad_3D / data.reprocess) - EVERY element of the [B,Ts,Tm] view is written.  The
 * reference calls its function with the two counts swapped against the parameter names (:409-413 vs :551), which is what this states:
 * n is the mel length, rows run over phonemes, the support point t = n is never emitted and rows do not sum to 1.  Evaluated in double
 * through lgamma, rounded once to float.  out is a view: element (b, s, t) lives at out[b stride_b + s stride_s + t] (strides in
 * floats, stride_s >= Tm, stride_b >= (Ts - 1) stride_s + Tm).  scaling_factor > 0, B <= 65535.
 *
 * ctts_outlier_stats: per utterance b over values[b][0 .. lens[b]): p25 / p75 = numpy's default (linear) percentile of the sorted
 * values (position q (n - 1), interpolated between the neighbours, in double); keep[b][i] = 1 iff p25 - 1.5 IQR < v < p75 + 1.5 IQR
 * (strict: a constant utterance and n = 1 keep nothing), 0 for i >= lens[b]; count[b], sum[b] and m2[b] = sum (v - sum / count)^2
 * over the kept values in double (two passes), vmin[b] / vmax[b] over the kept values (+inf / -inf when none is kept).
 * The dataset mean / std is the Chan merge of the (count, sum, m2) triples in utterance order = StandardScaler.partial_fit fed one
 * utterance at a time (ctts_amd.preprocess.merge_moments).  DOMAIN: 1 <= L <= 4096 (sorted in LDS; refused otherwise, never truncated). */
size_t ctts_trim_silence_workspace_bytes(int B, int N, int hop);
int ctts_trim_silence(const float* wav, const int32_t* lens, float* workspace, int32_t* start, int32_t* end, int B, int N, float top_db,
                      int frame_length, int hop, void* stream);
int ctts_attn_prior(const int32_t* src_lens, const int32_t* mel_lens, float* out, int B, int Ts, int Tm, int64_t stride_b, int64_t stride_s,
                    float scaling_factor, void* stream);
int ctts_outlier_stats(const float* values, const int32_t* lens, uint8_t* keep, int32_t* count, double* sum, double* m2, float* vmin,
                       float* vmax, int B, int L, void* stream);

/* ---------------------------------------------------------------------------------------
 * Objective evaluation on the device (csrc/metrics.hip): mel-cepstral distortion after dynamic-time-warping
 * alignment, log-F0 RMSE and voiced / unvoiced error of a synthesised utterance against its recording.  fp32 data, lengths are int32
 * device arrays, read once per workgroup and clamped to [0, padded size]; rows at or beyond a length are never read (they may hold
 * NaN).  Stream-ordered, no allocation, no host sync, no float atomics: every sum has one fixed order, bit-identical run to run.
 *
 * ctts_mel_cepstrum: mel [B][n_mel][F] (natural-log mel, the layout ctts_mel_spectrogram writes), frames [B] (NULL = F) ->
 * out [B][F][n_coef], out[b][f][k-1] = sqrt(2/M) sum_m mel[b][m][f] cos(pi k (m + 1/2) / M) for k = 1 .. n_coef, M = n_mel: the
 * orthonormal DCT-II over the mel axis with coefficient 0 dropped, terms added in channel order.  Rows f >= frames[b] are written as
 * zeros.  These are the DCT of THIS project's log-mel (MFCC-style cepstra), not WORLD / SPTK mel-cepstra.
 * DOMAIN: 1 <= n_coef <= 32, n_coef < n_mel, n_mel n_coef <= 12288, B <= 65535.
 *
 * ctts_dtw: x [B][Tx][K], y [B][Ty][K], x_lens / y_lens [B] -> cost [B], path_len [B], path [B][Tx + Ty - 1][2].
 *   align = 0: dynamic time warping.  Local cost d(i,j) = ||x_i - y_j||_2 (not squared); A(i,j) = d(i,j) + min(A(i-1,j-1), A(i-1,j),
 *   A(i,j-1)), A(0,0) = d(0,0); no window, no slope weights.  cost[b] = A(Lx-1, Ly-1).  The path is walked back from (Lx-1, Ly-1).
 *   TIE RULE: the diagonal (i-1,j-1) wins when it is <= both others, then (i-1,j), then (i,j-1).
 *   align = 1: no warping - frame i against frame i for i < min(Lx, Ly); cost[b] = sum_i d(i,i), the path is (i,i).
 *   path holds (i, j) pairs in order from (0,0); the first path_len[b] rows are filled and the kernel writes -1 into every other row.
 *   Lx = 0 or Ly = 0 gives cost 0, path_len 0 and an all -1 path.
 *   workspace: ctts_dtw_workspace_bytes(B, Tx, Ty) bytes, 32-byte aligned (the local costs as floats, one anti-diagonal per row of
 *   roundup(Tx, 8): [B][Tx + Ty - 1][roundup(Tx, 8)], then two direction bits per cell); align = 1 does not touch it (NULL allowed).
 *   DOMAIN: 1 <= Tx, Ty <= 2048 (padded sizes; refused before any launch otherwise), 1 <= K <= 32, B <= 65535.
 *
 * ctts_path_metrics: path [B][P][2], path_len [B] (clamped to P), f0_x [B][Tx], f0_y [B][Ty] in Hz with 0 = unvoiced (voiced: > 0) ->
 * out [B][4] double: the number of aligned pairs, the number voiced in both signals, the sum over those of
 * (1200 log2(f0_x[i] / f0_y[j]))^2 (cents squared, evaluated in double), the number of pairs whose voicing differs.  A row of the
 * path outside [0,Tx) x [0,Ty) is no pair and is skipped. */
size_t ctts_dtw_workspace_bytes(int B, int Tx, int Ty);
int ctts_mel_cepstrum(const float* mel, const int32_t* frames, float* out, int B, int n_mel, int F, int n_coef, void* stream);
int ctts_dtw(const float* x, const float* y, const int32_t* x_lens, const int32_t* y_lens, void* workspace, float* cost, int32_t* path_len,
             int32_t* path, int B, int Tx, int Ty, int K, int align, void* stream);
int ctts_path_metrics(const int32_t* path, const int32_t* path_len, const float* f0_x, const float* f0_y, double* out, int B, int Tx, int Ty,
                      int P, void* stream);

/* ---------------------------------------------------------------------------------------
 * Audio resampling on the device (csrc/resample.hip): the band-limited rate change behind every
 * librosa.load(path, sampling_rate) of the reference (preprocessor.py:364, :460, vctk.py:31) and the peak normalisation + int16 cast of
 * prepare_align (vctk.py:32-36).  fp32 data, lengths are int32 device arrays clamped to [0, N] in the kernels; stream-ordered, no
 * allocation, no host sync, no float atomics: bit-reproducible run to run, and a row's result does not depend on B, on the other rows
 * or on the launch geometry.
 *
 * ctts_resample: exact-phase polyphase FIR for the reduced ratio L / M (L up, M down).  wav [B][N], lens [B], bank [L][T] ->
 * out [B][No], No = ceil(N L / M), out_lens [B] = ceil(lens[b] L / M).  With t = n M + half, r = t mod L, k = t div L:
 *   out[b][n] = sum_{j = 0 .. T-1} bank[r][j] x_b[k - j],   x_b[i] = wav[b][i] for 0 <= i < lens[b], 0 elsewhere,
 * accumulated in fp32 with fmaf in the order j = 0, 1, .. T-1.  For a prototype filter h of 2 half + 1 taps the caller fills
 * bank[r][j] = h[r + j L] (0 beyond the last tap), which makes this out[n] = sum_k h[n M + half - k L] x[k]: PARITY with librosa /
 * resampy is UNPINNED (neither is installed where this project is built; resampy interpolates a filter table, this is exact-phase).
 *   EVERY element of out is written; columns at and beyond out_lens[b] are exactly 0.  Samples at and beyond lens[b] are never read.
 *   L == M copies (bank may be NULL, T and half are ignored).
 *   DOMAIN (refused before any launch, never truncated): 1 <= L, M <= 1024; T a multiple of 8 with 8 <= T <= 1024 and
 *   L T >= 2 half + 1; bank 32-byte aligned; B <= 65535; 1 <= N and No <= 2^30 (positions are formed in 64 bits).
 *   ctts_resample_tile(L, M, T, half): the number of consecutive outputs one tile of the kernel covers for these parameters (a
 *   multiple of L; 0 for L == M or parameters outside the domain) - it depends on nothing else, tests stand on its edges.
 *
 * ctts_peak_normalize: per utterance b, peak[b] = max |wav[b][i]| over i < lens[b];  v = (wav[b][i] / peak[b]) * max_wav_value as numpy
 * evaluates it on a float32 array (an IEEE division, then one multiply: two roundings);  q = trunc(v) saturated to [-32768, 32767];
 * out[b][i] = q / 32768 (what reading the written 16-bit file back gives), out_i16[b][i] = q (NULL: not wanted), 0 at and beyond
 * lens[b] - every element is written.  ONE deviation: the reference casts v = +32768.0 to int16, which is undefined in C and wraps to
 * -32768 on x86; here it saturates to 32767.  peak[b] == 0 (or lens[b] <= 0) gives zeros and valid[b] = 0 where the reference divides
 * by zero; valid[b] = 1 otherwise.  DOMAIN: finite samples, max_wav_value > 0, B <= 65535, N >= 1. */
int ctts_resample_tile(int L, int M, int T, int half);
int ctts_resample(const float* wav, const int32_t* lens, const float* bank, float* out, int32_t* out_lens, int B, int N, int L, int M, int T,
                  int half, void* stream);
int ctts_peak_normalize(const float* wav, const int32_t* lens, float* out, int16_t* out_i16, float* peak, int32_t* valid, int B, int N,
                        float max_wav_value, void* stream);

/* ---------------------------------------------------------------------------------------
 * Loudness on the device (csrc/loudness.hip): ITU-R BS.1770 gated loudness of mono utterances and the gain that
 * brings them to a target, what the reference does on the host with pyloudnorm (audio/stft.py:226-231).  PARITY with pyloudnorm is
 * UNPINNED (it is not installed where this project is built); the kernels are pinned against the float64 restatement in
 * tests/loudness_restate.py.  fp32 samples, lengths int32 device arrays clamped to [0, N]; every recursion state, product and sum is
 * double.  Stream-ordered, caller-allocated, no host sync, no float atomics, no workgroup waits on another: bit-reproducible, and a row's
 * result does not depend on B, on N, on the other rows or on the launch geometry.  Samples at and beyond lens[b] are never read.
 *
 * TABLES (made on the host, ctts_amd.loudness): a measurement is described by the sorted sample positions at which a block starts or
 * ends ("edges", edges[0] = 0, edges[n_edges - 1] = INT32_MAX), which cut the time axis into hop segments k = [edges[k], edges[k+1]);
 * chunk_seg[c], the segment that holds sample c * ctts_loudness_chunk(), for every chunk of every 64-chunk tile that starts below N; and
 * blocks[j] = {k0, k1}: block j is the union of segments k0 .. k1 - 1.  A tile may touch at most ctts_loudness_tile_slots() segments.
 * coef (double, ctts_loudness_coef_doubles() words): [0..4] b0 b1 b2 a1 a2 of the first section (a0 = 1), [5..9] of the second,
 * [16 + 16 (16 l + m - 1) ..] the row-major 4 x 4 matrix A^(chunk 16^l m), l = 0 .. 4, m = 1 .. 16, where A advances the state
 * (z1, z2 of section one, z1, z2 of section two; transposed direct form II) by one sample of zero input.
 *
 * ctts_kweight_energy: wav [B][N] -> hop_sums [B][ceil(N / (64 chunk))][slots] (double; sum of y^2 per tile and segment, y the K-weighted
 * signal; only tiles that start below lens[b] are written) and peak [B] = max |wav| over the utterance.  workspace:
 * ctts_loudness_workspace_bytes(B, N) bytes, 8-byte aligned.  Three launches: zero-state chunk responses, a per-utterance scan of the
 * chunk states with the powers in coef, the energy pass from the true states.  DOMAIN: B <= 65535, 1 <= N <= 2^24.
 *
 * ctts_loudness_gate: z_j = (sum of block j's segments) / block_samples for j < n_blocks[b]; l_j = -0.691 + 10 log10 z_j;
 * Gamma_r = -0.691 + 10 log10 mean{z_j : l_j >= -70} - 10; loudness[b] = -0.691 + 10 log10 mean{z_j : l_j > Gamma_r and l_j > -70}.
 * No such block: loudness = -inf, valid = 0, gain = 1.  Otherwise gain = 10^((target - loudness) / 20) rounded once to fp32, or, with
 * peak_limit and peak * gain > 1, the correctly rounded 1 / peak (x g / max |x g|).  curve [B][J] (NULL: not wanted) receives l_j, -inf
 * at and beyond n_blocks[b].  DOMAIN: J and n_edges - 2 at most ctts_loudness_max_segments().
 *
 * ctts_apply_gain: out[b][i] = wav[b][i] * gain[b] (one fp32 rounding) for i < lens[b], 0 beyond; every element written; out may be
 * wav.  16-byte accesses when N is a multiple of 4 and both pointers are 16-byte aligned. */
int ctts_loudness_chunk(void);
int ctts_loudness_tile_slots(void);
int ctts_loudness_coef_doubles(void);
int ctts_loudness_max_segments(void);
size_t ctts_loudness_workspace_bytes(int B, int N);
int ctts_kweight_energy(const float* wav, const int32_t* lens, const double* coef, const int32_t* edges, const int32_t* chunk_seg,
                        double* hop_sums, float* peak, int B, int N, int n_edges, int n_chunk_seg, void* workspace, void* stream);
int ctts_loudness_gate(const double* hop_sums, const int32_t* lens, const int32_t* n_blocks, const int32_t* edges, const int32_t* chunk_seg,
                       const int32_t* blocks, const float* peak, double* loudness, float* gain, int32_t* valid, double* curve, int B, int N,
                       int n_edges, int n_chunk_seg, int J, double block_samples, double target, int peak_limit, void* stream);
int ctts_apply_gain(const float* wav, const int32_t* lens, const float* gain, float* out, int B, int N, void* stream);

/* ---------------------------------------------------------------------------------------
 * Waveform metrics on the device (csrc/wavmetrics.hip): STOI / ESTOI, SI-SDR and the multi-resolution STFT
 * distances of a synthesised utterance `syn` against its sample-aligned recording `ref`, both [B][N] fp32 with one length per pair
 * (int32 device array, clamped to [0, N]).  The definitions are those of the ctts_amd.metrics docstring, pinned by the float64
 * restatement in tests/wavmetrics_restate.py; PARITY with pystoi is UNPINNED (it is not installed where this project is built, and it
 * resamples with another filter).  The samples enter exactly; every product, transform and sum is double.  Stream-ordered,
 * caller-allocated, no host sync, no float atomics, no workgroup waits on another: bit-reproducible, and a row's result does not depend
 * on B, on N, on the other rows or on the launch geometry.  Samples at and beyond lens[b] are never read.  Every output element is
 * written.  Workspaces are 8-byte aligned and need no initialisation.
 *
 * ctts_stoi: the signals are at 10 kHz.  window: the 256 doubles of the analysis window.  Frames of 256 at hop 128; the frames of ref
 * whose energy 20 log10(||w x_i|| + 2^-52) exceeds the largest one - 40 dB are kept, both signals' kept frames are windowed and
 * overlap-added (never materialised: the spectrum kernel gathers through the kept-index list), framed and windowed again, transformed
 * with 512 points and summed into 15 third-octave band amplitudes; every run of 30 such frames gives one STOI and one ESTOI value.
 * stoi [B], estoi [B]: their means, NaN without a segment or when ref's largest frame energy is 0.  counts [B][3]: frames, kept frames,
 * segments.  DOMAIN: B <= 65535; rows of N samples may hold at most ctts_stoi_max_frames frames (8192: 81.9 s, N <= 1048831); a
 * longer row is refused before any launch, and the workspace query returns 0 for it.
 *
 * ctts_si_sdr: out [B] = 10 log10(||t||^2 / ||y - t||^2) in dB with the means over [0, len) removed and t = (<y,x> / <x,x>) x, from
 * the five sums of x, y, xy, xx, yy (tiles of 4096 samples, then the tiles in index order).  NaN for len = 0 or <x,x> = 0, +inf where
 * the residual vanishes (y = 2^k x does so exactly).  DOMAIN: B <= 65535, N <= 2^30.
 *
 * ctts_mr_stft: one resolution of the Parallel-WaveGAN distances.  window: win doubles, zero-padded on the right to n_fft; frames start
 * at i hop for i < (len - win) / hop + 1, no padding; |X| = sqrt(max(re^2 + im^2, 1e-7)).  out [B][3]: spectral convergence
 * || |X| - |Y| ||_F / || |X| ||_F, mean | ln|X| - ln|Y| |, mean over frames of the root mean over bins of (20 log10|X| - 20 log10|Y|)^2;
 * NaN without a frame.  frames [B].  DOMAIN: n_fft 512, 1024 or 2048; 1 <= win <= n_fft; hop >= 1; B <= 65535; N <= 2^30. */
int ctts_stoi_max_frames(void);
size_t ctts_stoi_workspace_bytes(int B, int N);
int ctts_stoi(const float* ref, const float* syn, const int32_t* lens, const double* window, double* stoi, double* estoi, int32_t* counts,
              int B, int N, void* workspace, void* stream);
size_t ctts_si_sdr_workspace_bytes(int B, int N);
int ctts_si_sdr(const float* ref, const float* syn, const int32_t* lens, double* out, int B, int N, void* workspace, void* stream);
size_t ctts_mr_stft_workspace_bytes(int B, int N, int hop, int win);
int ctts_mr_stft(const float* ref, const float* syn, const int32_t* lens, const double* window, double* out, int32_t* frames, int B, int N,
                 int n_fft, int hop, int win, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------
 * Speaker embeddings on the device (csrc/speaker.hip): the DeepSpeaker front end and ResCNN.  The definitions are
 * those of the ctts_amd.speaker docstring, pinned by the float64 restatement in tests/speaker_restate.py; PARITY with the TF model and
 * python_speech_features is UNPINNED (neither is installed where this project is built).  Stream-ordered, caller-allocated, no host
 * sync, no float atomics: bit-reproducible, and a row's result does not depend on the other rows.  Every output element is written.
 *
 * Span: wav [B][N] fp32, lens int32 [B] (clamped to [0, N]; samples at and beyond lens[b] are never read).  thr = the 95th percentile of
 * |x| with linear interpolation, formed in double from the two fp32 order statistics the way numpy forms it; first / last = the lowest /
 * highest index with |x| > thr in double (both 0 when there is none); valid = last - first >= 1; n_frames = the frame count of the span
 * x[first:last] (frames of 551 at step 221, the tail zero-padded: 1 up to 551 samples, else 1 + ceil((L - 551) / 221)), 0 when invalid.
 * The frame-count query returns that count for a span of L samples.
 *
 * Fbank: out [B][out_frames][64] fp32.  Row j holds frame r + j of the span: pre-emphasis 0.97 inside the span, rectangular window,
 * |rfft(frame, 1024)|^2 / 1024, the 64 triangular filters on `bins` (int32 [66], non-decreasing in [0, 512]), exact zeros replaced by
 * 2^-52, then (v - mean) / max(std, 1e-12) over the 64 filters (population std); computed in double, rounded once.  r = offsets[b]
 * (int32 [B]) when given, else (n_frames - out_frames) / 2 when `centre`, else 0; clamped to [0, max(n_frames - out_frames, 0)].  Rows
 * at and beyond n_frames, and every row of an invalid utterance, are zeros.
 *
 * Conv: NHWC fp32 x [B][H][W][Cin] -> out [B][Ho][Wo][Cout], weights [kh][kw][Cin][Cout] (the Keras layout), as an implicit GEMM on the
 * exact fp32 MFMA - no patch matrix in memory.  geom 0: 5 x 5, stride 2, TF 'same' (Ho = ceil(H / 2); total = max((Ho - 1) 2 + 5 - H, 0)
 * cells of padding, total / 2 of them before: even sizes pad (1, 2), odd ones (2, 2));  geom 1: 3 x 3, stride 1, pad 1.  mode 0:
 * clip(acc + bias);  mode 1: clip(clip(acc + bias) + res) with res shaped like out;  clip(v) = min(max(v, lo), hi).  DOMAIN: B, H, W >= 1,
 * Cin 1 or a multiple of 64, Cout a multiple of 64, fewer than 2^31 elements in x and in out, 16-byte aligned pointers.  Shapes with few
 * output tiles split K; their partial tiles go through `workspace` (size from the query, 0 when none is needed; no initialisation) and
 * are added in index order.
 *
 * Head: x [B][T][F] -> out [B][E]: the mean over T, times w [F][E] plus bias [E], divided by max(its L2 norm, 1e-12); sums in double.
 * Rows with valid[b] == 0 are zeros (valid may be NULL).  DOMAIN: F + E <= 7168. */
int ctts_speaker_frames(int span);
int ctts_speaker_span(const float* wav, const int32_t* lens, int32_t* first, int32_t* last, int32_t* n_frames, int32_t* valid, int B, int N,
                      void* stream);
int ctts_speaker_fbank(const float* wav, const int32_t* first, const int32_t* last, const int32_t* valid, const int32_t* bins,
                       const int32_t* offsets, float* out, int B, int N, int out_frames, int centre, void* stream);
size_t ctts_conv2d_nhwc_workspace_bytes(int B, int H, int W, int Cin, int Cout, int geom);
int ctts_conv2d_nhwc(const float* x, const float* w, const float* bias, const float* res, float* out, int B, int H, int W, int Cin, int Cout,
                     int geom, int mode, float lo, float hi, void* workspace, void* stream);
int ctts_speaker_head(const float* x, const float* w, const float* bias, const int32_t* valid, float* out, int B, int T, int F, int E,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
