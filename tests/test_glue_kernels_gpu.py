"""GPU: the glue kernels between the GEMMs - the length regulator (index, gather, segment-sum gradient), positions and the embedding
lookup with its weight gradient (csrc/lr.hip), and rowscale_dropout, act_dropout_bwd, epilogue_bwd, colsum, weighted_colsum, the
positional-embedding add and the deferred partial sums (csrc/elementwise.hip) - against the restatement tests/glue_restate64.py, at the
sizes where a 64-lane carry, a search loop, a grid, a stripe plan, a ticket level, a fold or an alignment path changes.

Exact (torch.equal): lr_index (mel2ph, mel_len, cum), lr_gather_fwd, positions, embedding_fwd, rowscale_dropout, the posembed forward
(against the restatement run in float32: two roundings), the dx of posembed_bwd, gm of epilogue_bwd and dz of an epilogue without
activation.  The dropout mask is tests/gemm_restate64.keep_mask, never a mask drawn from a kernel.

Error measure of the sums (never the tensor's global maximum): element by element against the L2 norm of the float64 summands, plus
|old| for an accumulating call; dz = g * act'(z) element by element against |g| = |dy * rowscale * drop|.  A reference of exactly zero
(a phoneme of 0 frames, an id that never occurs, a dropped element) must be met exactly.
Bar of every measured quantity: max(FACTOR x the error of the same restatement run in float32 on the CPU (same input, same measure),
4 * 2^-23).  FACTOR = 8 and the floor are the constants of tests/test_seq_kernels_gpu.py, INHERITED and not measured for these
kernels.  Every comparison prints `kernel err / stock float32 err / bar` (run with -s).  WIDER holds the quantities that need
another factor, with the measured ratio and the reason.

Paths reached, from the launch arithmetic of lr.hip and elementwise.hip:
  lr_index         1 .. 4 scan chunks (Ts 1 .. 200), 1 .. 3 trips of the 256-thread search (Tm 257, 600), both input types and roundings
  lr_gather_fwd    grid of 1 .. 2048 workgroups, the second trip of the grid-stride loop (563200 float4); _bwd: one trip only (8320 float4;
                   a second trip needs B * Ts * C / 4 > 524288 and the issue fixes Ts = 65)
  positions        1 .. 3 chunks, int64 and float32 with stride 3
  embedding_fwd    one trip (the 4096-workgroup cap needs more than a million float4)
  embedding_bwd    NC 1 (C 4, 64), 4 (68, 256), 8 (260, 512, 384); NG 1 (n <= 4032, and V 1025 without a workspace), 2 (4095, 4096), 8 (16384,
                   16385); 1 .. 16 trips of the four-rows-in-flight loop (all ids equal)
  dropout kernels  scalar path (C 1, 2, 11; rows * C odd for act_dropout_bwd) and float4 path; grid-stride second trips are NOT reached
                   (they need more than 8192 * 256 float4 per launch)
  posembed_bwd     1, 1 and 18 workgroups: no ticket, and two ticket levels (groups of 16 + 2)
  epilogue_bwd     1 stripe (rows 1 .. 33), 3 (rows 100: one level), 18 (rows 600: two levels, G 16), 1025 (rows 32800: G 32, 33 groups); 1 and 4
                   column blocks; deferred partial rows (18)
  colsum           fold k 64, 32, 16, 8, 2 and 1; 1, 15 (one level) and 17 stripes (two levels); 1, 2 and 16 column blocks; ld > C; deferred (17);
                   G 32 is reached through epilogue_bwd only (colsum would need 65600 rows); weighted_colsum: the same stripes, never folded
  partial_sums     aligned and scalar path with every count of 1, 7, 8, 9, the scalar tail of an aligned task, a task over 2 workgroups, 24 + 1
                   tasks; one chunk trip per workgroup except task 0 (PSUM_CHUNKS trips)

No quantity needed a wider factor (WIDER stays empty).  The largest kernel / float32 ratio is 14 (weighted_colsum [1089, 1]: 1.2e-7
against 8.6e-9, the fmaf chain of four row phases against torch's blocked sum), there and wherever the ratio passes 8 the floor is the
bar; gather, embedding, partial sums and dalpha add in the restatement's own order or a more balanced one and never pass 1.0 x float32.

Measured on the MI355X, worst case per quantity by its share of the bar (kernel error / stock float32 error / bar; 1173 comparisons, none
above 0.42 of its bar):
  lr_gather_bwd dx       1.4e-6 / 1.4e-6 / 1.1e-5 (one phoneme of 300 frames, C 256: the same frame-after-frame order)
  embedding_bwd dw       2.2e-7 / 2.2e-7 / 1.8e-6 (n 64, C 64, accumulate)
  posembed_bwd dalpha    9.1e-8 / 9.0e-8 / 7.2e-7 ([16, 64], accumulate)
  act_dropout_bwd dz     1.4e-7 / 2.6e-8 / 4.8e-7 ([1, 11] GELU: 5.3 x float32, ctts_erf and __expf; the floor is the bar)
  epilogue_bwd dz        2.4e-7 / 1.4e-7 / 1.2e-6 ([33, 11] GELU)
  epilogue_bwd dbias     5.7e-7 / 2.6e-7 / 2.1e-6 ([32, 200] GELU, one stripe)   deferred, 18 stripes: 4.3e-7 / 3.3e-7 / 2.6e-6
  colsum                 3.3e-7 / 1.0e-7 / 8.1e-7 ([96, 2] folded 32-fold, accumulate)   deferred, 17 stripes: 2.3e-7 / 5.1e-7 / 4.1e-6
  weighted_colsum        2.0e-7 / 1.4e-8 / 4.8e-7 ([1089, 3], accumulate)   deferred, 17 stripes: 3.3e-7 / 3.5e-7 / 2.8e-6
  partial_sums           1.4e-7 / 1.4e-7 / 1.1e-6 (n 73, 7 partials)
  bit-exact              lr_index (750 launches), lr_gather_fwd, positions, embedding_fwd, rowscale_dropout, posembed forward and dx,
                         epilogue_bwd gm and dz without activation, at every shape
"""
import math

import pytest
import torch

import ctts_amd  # noqa: F401
from ctts_amd import kernels as K
from tests import glue_restate64 as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 4 * 2.0 ** -23
FACTOR = 8.0
TINY = 1e-300
D, F32 = torch.float64, torch.float32
WIDER = {}                                            # quantity -> widened factor
SENTINEL = -12345.678
OFFSET = 3                                            # the dropout call-site offset of every case


def dev(t):
    return None if t is None else t.to(DEV)


def c64(t):
    return t.detach().double().cpu()


def err_scaled(got, ref64, scale):
    """worst |got - ref64| / scale, element for element (scale 0: the element must be met exactly)"""
    got, ref64 = c64(got), c64(ref64)
    assert got.shape == ref64.shape == scale.shape, (got.shape, ref64.shape, scale.shape)
    return ((got - ref64).abs() / scale.double().clamp_min(TINY)).max().item() if got.numel() else 0.0


def check_scaled(quantity, tag, got, r64, r32, scale):
    assert torch.isfinite(got).all(), (quantity, tag)
    e, e32 = err_scaled(got, r64, scale), err_scaled(r32, r64, scale)
    bar = max(WIDER.get(quantity, FACTOR) * e32, FLOOR)
    print(f"{quantity} [{tag}]: kernel err {e:.2e}  stock float32 {e32:.2e}  bar {bar:.2e}")
    assert math.isfinite(e) and e <= bar, f"{quantity} [{tag}]: kernel err {e:.3e} > bar {bar:.3e} (stock float32 {e32:.3e})"


def same(got, want, what):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert torch.equal(got, want), f"{what}: {(got != want).sum().item()} of {want.numel()} elements differ"


def drop_ctx():
    ctx = K.DropCtx(DEV, seed=9)
    return ctx.seed, int(ctx.seed.item()) & 0xFFFFFFFFFFFFFFFF


def guarded(init):
    """(buffer with 64 sentinel floats behind a copy of `init`, the view of that copy)"""
    buf = torch.full((init.numel() + 64,), SENTINEL, device=DEV)
    view = buf[:init.numel()].view(init.shape)
    view.copy_(init)
    return buf, view


def guard_ok(buf, n):
    return bool((buf[n:] == SENTINEL).all())


# ================================================================================================ length regulator
@pytest.mark.parametrize("Ts", S.LR_TS)
def test_lr_index_is_exact(Ts):
    """int64 and float32 durations, trunc and round-half-even, no pad / uint8 pad / bool pad, Tm around row 0's total and past the
    256-thread search loop; Ts around the 64-lane chunks of the scan: mel2ph, mel_len and cum equal the model's, integer for integer"""
    n = 0
    for kind, dur in (("int64", S.lr_int_durations(Ts)), ("int64 above the cap", S.lr_int_durations(Ts, big=True)),
                      ("float32", S.lr_float_durations(Ts))):
        u8 = S.lr_pad(Ts)
        for rm in (0, 1):
            for pname, pad in (("none", None), ("uint8", u8), ("bool", u8.bool())):
                total = int(S.lr_index(dur, 1, pad, rm)[1][0])
                assert total >= 1
                for Tm in S.lr_tm_set(total):
                    want = S.lr_index(dur, Tm, pad, rm)
                    got = K.lr_index(dev(dur), Tm, dev(pad), rm)
                    for g, w, q in zip(got, want, ("mel2ph", "mel_len", "cum")):
                        same(g, w, f"lr_index {q} [{kind} Ts {Ts} Tm {Tm} round {rm} pad {pname}]")
                    n += 1
        m2, mel_len, cum = K.lr_index(dev(dur), 5, None, 0, want_mel2ph=False)
        want = S.lr_index(dur, 5)
        assert m2 is None
        same(mel_len, want[1], f"lr_index mel_len without mel2ph [{kind} Ts {Ts}]")
        same(cum, want[2], f"lr_index cum without mel2ph [{kind} Ts {Ts}]")
    print(f"lr_index [Ts {Ts}]: {n} launches exact")


def test_lr_index_does_not_wrap_past_int32():
    """two durations of 2e9 (int64) / +inf (float32) in one row, at elements 3 and 64: mel2ph is 4 at every frame, cum saturates at
    2^31 - 1 and mel_len is the exact total 4e9.  Only lr_index runs: it writes cum[i < Ts] and mel2ph[t < Tm] whatever the durations."""
    Tm = 300
    for dur in S.lr_overflow_durations():
        want = S.lr_index(dur, Tm)
        assert (want[0] == 4).all() and int(want[1][0]) == 4_000_000_000 and int(want[2][0, 64]) == S.INT32_MAX and int(want[2][0, 3]) == S.DUR_CAP
        got = K.lr_index(dev(dur), Tm)
        for g, w, q in zip(got, want, ("mel2ph", "mel_len", "cum")):
            same(g, w, f"lr_index {q} [overflow {dur.dtype}]")


def _gather_fwd_case(B, Ts, C, Tm, dur):
    x = S.randn(B, Ts, C, seed=Tm)
    mel2ph = S.lr_index(dur, Tm)[0]
    same(K.lr_gather_fwd(dev(x), dev(mel2ph)), S.lr_gather(x, mel2ph, F32), f"lr_gather_fwd [B {B} Ts {Ts} C {C} Tm {Tm}]")


@pytest.mark.parametrize("B,Ts,C", S.GATHER_FWD_CASES)
def test_lr_gather_forward_is_a_copy(B, Ts, C):
    """Tm in the middle of a run, Tm beyond the total (zero rows); a phoneme of 0 frames is never copied"""
    dur = S.gather_durations(B, Ts)
    for Tm in S.gather_fwd_tms(dur):
        _gather_fwd_case(B, Ts, C, Tm, dur)


def test_lr_gather_forward_grid_stride_loop():
    B, Ts, C, Tm = S.GATHER_FWD_LOOP
    assert B * Tm * (C // 4) > 2048 * 256
    _gather_fwd_case(B, Ts, C, Tm, S.gather_durations(B, Ts))


@pytest.mark.parametrize("C", [4, 256])
@pytest.mark.parametrize("case", ["crop", "long"])
def test_lr_gather_gradient_against_float64(case, C):
    """Ts = 65; `crop`: Tm cuts a run in the middle, the phonemes behind it get exactly 0; `long`: one phoneme of 300 frames; both hold
    phonemes of 0 frames, whose dx row must be exactly 0"""
    B, Ts = 2, S.GATHER_BWD_TS
    dur = S.gather_durations(B, Ts, seed=1, long_run=300 if case == "long" else 0)
    inside, beyond = S.gather_fwd_tms(dur)
    Tm = inside if case == "crop" else beyond
    cum = S.lr_index(dur, Tm)[2]
    dy = S.randn(B, Tm, C, seed=C)
    (r64, norm), (r32, _) = [S.lr_gather_grad(dy, cum, dtype=t) for t in (D, F32)]
    assert (norm[:, Ts // 2] == 0).all(), "the case needs a phoneme of 0 frames"
    dx = K.lr_gather_bwd(dev(dy), dev(cum), Ts)
    check_scaled("lr_gather_bwd dx", f"{case} Tm {Tm} C {C}", dx, r64, r32, norm)
    assert (dx[:, Ts // 2] == 0).all()


# ================================================================================================ positions, embedding
@pytest.mark.parametrize("T", S.POSITIONS_T)
def test_positions_are_exact(T):
    """the carry between the 64-lane chunks: zeros at the chunk boundaries, an all-zero row, negative ids, leading zeros; the float
    path tests channel 0 only (stride = C), -0.0 is zero and NaN is not"""
    s = S.positions_int_input(T)
    same(K.positions(dev(s)), S.positions(s), f"positions int64 [T {T}]")
    x = S.positions_float_input(T)
    same(K.positions(dev(x), x.shape[2]), S.positions(x, x.shape[2]), f"positions float32 [T {T}]")


@pytest.mark.parametrize("C", [4, 64])
def test_embedding_forward_is_a_copy(C):
    """ids -1 and V give zero rows"""
    V = 7
    ids = torch.randint(0, V, (3, 50), generator=torch.Generator().manual_seed(C))
    ids[0, 0], ids[1, 7], ids[2, 49], ids[2, 48] = -1, V, V, 0
    w = S.randn(V, C)
    same(K.embedding_fwd(dev(ids), dev(w)), S.embedding(ids, w, F32), f"embedding_fwd [C {C}]")


def _embedding_bwd_case(n, C, V, kind="mixed", pads=None):
    ids, dy, old = S.embedding_ids(n, V, kind), S.randn(n, C, seed=1), S.randn(V, C, seed=2)
    for pad in ((-1, 0, V - 1, V) if pads is None else pads):
        for acc in (False, True):
            (r64, norm), (r32, _) = [S.embedding_grad(ids, dy, V, pad, old if acc else None, dtype=t) for t in (D, F32)]
            tag = f"n {n} C {C} V {V} {kind} padding_idx {pad} {'accumulate' if acc else 'overwrite'}"
            buf, view = guarded(old)
            got = K.embedding_bwd(dev(ids), dev(dy), V, pad, acc_into=view) if acc else K.embedding_bwd(dev(ids), dev(dy), V, pad)
            if acc:
                assert guard_ok(buf, V * C), f"embedding_bwd wrote past V * C floats [{tag}]"
            check_scaled("embedding_bwd dw", tag, got, r64, r32, norm)
            unused = [v for v in range(V) if v == pad or not (ids == v).any()]
            assert unused, "the case needs a row that gets no gradient"
            want = old[unused] if acc else torch.zeros(len(unused), C)
            same(got[unused], want, f"embedding_bwd rows without a gradient [{tag}]")


@pytest.mark.parametrize("C", S.EMB_C)
@pytest.mark.parametrize("n", S.EMB_N)
def test_embedding_gradient_against_float64(n, C):
    """n around one 64-id chunk and around the step from one group of chunks to several; C at the edges of the three per-lane widths;
    padding_idx absent, first row, last row, V; overwrite and accumulate; id V // 2 never occurs and ids -1, V, V + 3 do"""
    _embedding_bwd_case(n, C, S.EMB_V)


def test_embedding_gradient_all_ids_equal():
    """one row takes every position (the unvoiced pitch bin): all the others are exactly 0 or unchanged"""
    _embedding_bwd_case(4096, 64, S.EMB_V, kind="equal", pads=(-1, 1))


@pytest.mark.parametrize("C", [4, 68])
def test_embedding_gradient_large_vocabulary(C):
    """V = 1025 > 1024: one workgroup per row, no workspace"""
    _embedding_bwd_case(65, C, 1025, pads=(-1, 0))


def test_embedding_gradient_at_the_pitch_embedding_shape():
    _embedding_bwd_case(16384, 384, S.EMB_V, pads=(-1, 0))


# ================================================================================================ dropout kernels, exact
@pytest.mark.parametrize("p", S.DROP_P)
@pytest.mark.parametrize("C", S.DROP_C)
def test_dropout_kernels_are_exact(C, p):
    """rowscale_dropout, posembed forward and dx (C % 4 == 0), epilogue_bwd gm and its dz without activation: bit-identical to the
    restatement run in float32 with the restated mask; C = 1, 2, 11 take the scalar paths"""
    rows = S.DROP_ROWS
    seed, seed_u64 = drop_ctx()
    x, rs = S.randn(rows, C, seed=4), S.rowscale_input(rows)
    drop = S.drop_scale(seed_u64, OFFSET, p, rows, C, F32)
    if p > 0:
        assert (drop == 0).any() and (drop != 0).any()
    tag = f"[{rows}, {C}] p {p}"
    for rsn, r in (("", None), (" rowscale", rs)):
        same(K.rowscale_dropout(dev(x), dev(r), p, seed, OFFSET), S.rowscale_dropout(x, r, drop, F32), f"rowscale_dropout {tag}{rsn}")
        dz, gm, _ = K.epilogue_bwd(dev(x), dev(r), None, 0, p, seed, OFFSET, want_gm=True)
        ref = S.epilogue_bwd(x, r, None, 0, drop, dtype=F32)
        same(gm, ref["gm"], f"epilogue_bwd gm {tag}{rsn}")
        same(dz, ref["dz"], f"epilogue_bwd dz without activation {tag}{rsn}")
    if C % 4 == 0:
        pos = torch.randint(0, 12, (rows,), generator=torch.Generator().manual_seed(C)).to(torch.int32)
        table, alpha = S.randn(12, C, seed=5), torch.tensor([0.7])
        for a in (None, alpha):
            same(K.posembed_fwd(dev(x), dev(pos), dev(table), dev(a), dev(rs), p, seed, OFFSET), S.posembed(x, pos, table, a, rs, drop, F32),
                 f"posembed_fwd {tag} alpha {a is not None}")
        dx, dalpha = K.posembed_bwd(dev(x), dev(pos), dev(table), dev(rs), p, seed, OFFSET, want_alpha=False)
        assert dalpha is None
        same(dx, S.posembed_grad(x, pos, table, rs, drop, dtype=F32)[0], f"posembed_bwd dx {tag}")


# ================================================================================================ posembed dalpha
@pytest.mark.parametrize("rows,C", S.DALPHA_SHAPES)
def test_posembed_alpha_gradient_against_float64(rows, C):
    """rows * C / 4 = 1, 256, 4480: one workgroup, one full workgroup, 18 workgroups (two ticket levels); pos holds 0, rowscale has
    zero rows; overwrite and alpha_acc_into; without the alpha gradient dx is unchanged"""
    seed, seed_u64 = drop_ctx()
    dy, rs = S.randn(rows, C, seed=6), S.rowscale_input(rows)
    pos = torch.randint(0, 9, (rows,), generator=torch.Generator().manual_seed(rows)).to(torch.int32)
    pos[0] = 0
    table = S.randn(9, C, seed=7)
    table[0] = 0.0                                                     # the padding position's row of the sinusoid table
    old = torch.tensor([0.37])
    for p in (0.0, 0.1):
        drop64, drop32 = [S.drop_scale(seed_u64, OFFSET, p, rows, C, t) for t in (D, F32)]
        for r in (None, rs):
            tag = f"[{rows}, {C}] p {p} rowscale {r is not None}"
            for acc in (None, old):
                (_, a64, norm), (dx32, a32, _) = [S.posembed_grad(dy, pos, table, r, d, acc, dtype=t) for t, d in ((D, drop64), (F32, drop32))]
                into = dev(acc.clone()) if acc is not None else None
                dx, dalpha = K.posembed_bwd(dev(dy), dev(pos), dev(table), dev(r), p, seed, OFFSET, alpha_acc_into=into)
                same(dx, dx32, f"posembed_bwd dx {tag}")
                check_scaled("posembed_bwd dalpha", f"{tag} {'accumulate' if acc is not None else 'overwrite'}", dalpha, a64, a32, norm)


# ================================================================================================ act_dropout_bwd, epilogue_bwd
def _epilogue_case(rows, C, act, p, tag_extra=""):
    seed, seed_u64 = drop_ctx()
    dy, z, rs, old = S.randn(rows, C, seed=8), S.act_z(rows, C), S.rowscale_input(rows), S.randn(C, seed=9)
    drop64, drop32 = [S.drop_scale(seed_u64, OFFSET, p, rows, C, t) for t in (D, F32)]
    tag = f"[{rows}, {C}] act {act} p {p}{tag_extra}"
    (a64, ascale), (a32, _) = [S.act_dropout_bwd(dy, z, act, d, dtype=t) for t, d in ((D, drop64), (F32, drop32))]
    check_scaled("act_dropout_bwd dz", tag, K.act_dropout_bwd(dev(dy), dev(z), act, p, seed, OFFSET), a64, a32, ascale)
    for acc in (None, old):
        r64, r32 = [S.epilogue_bwd(dy, rs, z, act, d, 2.0, acc, dtype=t) for t, d in ((D, drop64), (F32, drop32))]
        buf, view = guarded(old)
        dz, gm, dbias = K.epilogue_bwd(dev(dy), dev(rs), dev(z), act, p, seed, OFFSET, want_gm=True, want_bias=True, bias_scale=2.0,
                                       bias_acc_into=view if acc is not None else None)
        assert acc is None or (dbias is view and guard_ok(buf, C)), f"epilogue_bwd wrote past C floats {tag}"
        same(gm, r32["gm"], f"epilogue_bwd gm {tag}")
        check_scaled("epilogue_bwd dz", tag, dz, r64["dz"], r32["dz"], r64["dz_scale"])
        check_scaled("epilogue_bwd dbias", f"{tag} {'accumulate' if acc is not None else 'overwrite'}", dbias, r64["dbias"], r32["dbias"],
                     r64["dbias_norm"])


@pytest.mark.parametrize("rows", S.EPI_ROWS)
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_activation_backward_and_bias_gradient_against_float64(act, rows):
    """z holds exact 0, +-1e-3, +-20 and a random body; rows around the 32-row stripe, 100 rows = 3 stripes, 600 rows = 18 stripes (two ticket levels); C = 11
    (scalar path of act_dropout_bwd at odd rows) and 200 (four column blocks, the last with 8 columns); dbias = 2 * column sums of the
    RESTATED dz, overwriting and accumulating"""
    for C in S.EPI_C:
        for p in (0.0, 0.1):
            _epilogue_case(rows, C, act, p)


def test_bias_gradient_over_1025_stripes():
    """rows = 32800, C = 8: 1025 stripes, ticket groups of 32"""
    _epilogue_case(32800, 8, 2, 0.1)


# ================================================================================================ colsum, weighted_colsum
def _colsum_case(x_full, c0, C, tag):
    """the view x_full[:, c0:c0 + C] (ld = x_full.shape[1]); scale 1 / overwrite and scale -0.5 / accumulate, plain and weighted"""
    rows, ld = x_full.shape
    xv = x_full[:, c0:c0 + C]
    xd = dev(x_full)[:, c0:c0 + C]
    w, old = S.randn(rows, seed=10), S.randn(C, seed=11)
    for scale, acc in ((1.0, None), (-0.5, old)):
        mode = "accumulate" if acc is not None else "overwrite"
        (r64, norm), (r32, _) = [S.colsum(xv, scale, acc, dtype=t) for t in (D, F32)]
        buf, view = guarded(old)
        got = K.colsum(xd, ld=ld, scale=scale, acc_into=view if acc is not None else None)
        assert guard_ok(buf, C), f"colsum wrote past C floats {tag}"
        check_scaled("colsum", f"{tag} scale {scale} {mode}", got, r64, r32, norm)
        if ld == C:
            (r64, norm), (r32, _) = [S.weighted_colsum(xv, w, scale, acc, dtype=t) for t in (D, F32)]
            buf, view = guarded(old)
            got = K.weighted_colsum(xd, dev(w), scale=scale, acc_into=view if acc is not None else None)
            assert guard_ok(buf, C), f"weighted_colsum wrote past C floats {tag}"
            check_scaled("weighted_colsum", f"{tag} scale {scale} {mode}", got, r64, r32, norm)


@pytest.mark.parametrize("rows", S.COLSUM_ROWS)
@pytest.mark.parametrize("C", S.COLSUM_NARROW_C)
def test_narrow_column_sums_against_float64(C, rows):
    """dense narrow matrices are folded k-fold into 64-wide rows: rows = 64 * 17 folds fully, 64 * 17 + 1 not at all, 96 and 1000 in part"""
    _colsum_case(S.randn(rows, C, seed=12), 0, C, f"[{rows}, {C}] fold {S.colsum_fold(rows, C)}")


@pytest.mark.parametrize("rows", [1000, 64 * 17])
@pytest.mark.parametrize("C", S.COLSUM_WIDE_C)
def test_wide_column_sums_against_float64(C, rows):
    """one full column block, a second block of one column, 16 blocks of which the last holds 40 columns; 15 and 17 stripes"""
    _colsum_case(S.randn(rows, C, seed=13), 0, C, f"[{rows}, {C}]")


@pytest.mark.parametrize("C", [5, 32, 65])
def test_column_sums_of_a_column_slice_against_float64(C):
    """ld > C: columns 3 .. 3 + C of a [1088, C + 7] matrix; a narrow slice is not folded"""
    _colsum_case(S.randn(64 * 17, C + 7, seed=14), 3, C, f"[1088, {C}] of ld {C + 7}")


# ================================================================================================ deferred sums
def _with_sink(fn):
    sink = K.PartialSink()
    prev = K.set_partial_sink(sink)
    try:
        fn(sink)
    finally:
        K.set_partial_sink(prev)


def test_partial_sums_of_one_flush_against_float64():
    """25 tasks in one flush (two launches: 24 + 1): counts 1, 7, 8, 9 (the 8-deep pipeline of the aligned path), a task over two
    workgroups, destinations one float into their buffer, a stride that is no multiple of 4 and tails of fewer than 4 elements (scalar
    path); every destination sits between guard cells"""
    sink = K.PartialSink()
    sink.FLUSH_BYTES = 0
    made = []
    for t, (n, count, stride, off) in enumerate(S.psum_tasks()):
        src, old, alpha = S.randn(count * stride, seed=20 + t), S.randn(n, seed=50 + t), (1.0, -0.5, 2.0)[t % 3]
        buf = torch.full((n + off + 64,), SENTINEL, device=DEV)
        buf[off:off + n] = dev(old)
        srcd = dev(src)
        sink.add(srcd, count, stride, n, buf, alpha, 0, off)
        made.append((t, n, count, stride, off, src, old, alpha, buf))
    assert len(sink.tasks) == 25
    sink.flush()
    for t, n, count, stride, off, src, old, alpha, buf in made:
        (r64, norm), (r32, _) = [S.partial_sums(old, src, count, stride, n, alpha, dtype=d) for d in (D, F32)]
        assert (buf[:off] == SENTINEL).all() and (buf[off + n:] == SENTINEL).all(), f"task {t} wrote outside its destination"
        check_scaled("partial_sums", f"task {t} n {n} count {count} stride {stride} offset {off} alpha {alpha}", buf[off:off + n], r64, r32, norm)


def test_deferred_column_sums_against_float64(monkeypatch):
    """colsum, weighted_colsum and the bias gradient of epilogue_bwd under a PartialSink: the kernels write their stripes' partial rows
    and the flush adds them in order; a narrow even-rowed colsum has no deferred mode (ctts_reduce_parts = 0) and must still finish at
    once, and right"""
    monkeypatch.setattr(K, "DEFER_ENABLED", True)
    seed, seed_u64 = drop_ctx()
    rows, C = 64 * 17, 65
    x, w, old = S.randn(rows, C, seed=30), S.randn(rows, seed=31), S.randn(C, seed=32)
    er, ec, p, act = 600, 200, 0.1, 2
    dy, z, rs, eold = S.randn(er, ec, seed=33), S.act_z(er, ec), S.rowscale_input(er), S.randn(ec, seed=34)
    nx, nold = S.randn(96, 2, seed=35), S.randn(2, seed=36)
    out = {}

    def run(sink):
        for name, o in (("colsum", old), ("weighted", old), ("dbias", eold), ("narrow", nold)):
            out[name] = guarded(o)
        K.colsum(dev(x), scale=-0.5, acc_into=out["colsum"][1])
        assert len(sink.tasks) == 1 and sink.tasks[-1][4] == 17, "colsum [1088, 65] defers 17 stripes"
        K.weighted_colsum(dev(x), dev(w), scale=2.0, acc_into=out["weighted"][1])
        assert len(sink.tasks) == 2 and sink.tasks[-1][4] == 17
        out["dz"] = K.epilogue_bwd(dev(dy), dev(rs), dev(z), act, p, seed, OFFSET, want_bias=True, bias_scale=2.0, bias_acc_into=out["dbias"][1])[0]
        assert len(sink.tasks) == 3 and sink.tasks[-1][4] == 18, "epilogue_bwd [600, 200] defers 18 stripes"
        K.colsum(dev(nx), acc_into=out["narrow"][1])
        assert len(sink.tasks) == 3, "a folded colsum has no deferred mode"
        (r64, norm), (r32, _) = [S.colsum(nx, 1.0, nold, dtype=t) for t in (D, F32)]
        check_scaled("colsum", "[96, 2] immediate under a sink", out["narrow"][1], r64, r32, norm)
        sink.flush()

    _with_sink(run)
    for name, ref in (("colsum", lambda t: S.colsum(x, -0.5, old, dtype=t)), ("weighted", lambda t: S.weighted_colsum(x, w, 2.0, old, dtype=t))):
        (r64, norm), (r32, _) = ref(D), ref(F32)
        assert guard_ok(out[name][0], C)
        check_scaled(f"deferred {name}", f"[{rows}, {C}] 17 stripes", out[name][1], r64, r32, norm)
    r64, r32 = [S.epilogue_bwd(dy, rs, z, act, S.drop_scale(seed_u64, OFFSET, p, er, ec, t), 2.0, eold, dtype=t) for t in (D, F32)]
    assert guard_ok(out["dbias"][0], ec) and guard_ok(out["narrow"][0], 2)
    check_scaled("epilogue_bwd dz", f"[{er}, {ec}] deferred", out["dz"], r64["dz"], r32["dz"], r64["dz_scale"])
    check_scaled("deferred dbias", f"[{er}, {ec}] 18 stripes", out["dbias"][1], r64["dbias"], r32["dbias"], r64["dbias_norm"])
