"""GPU: the fused attention kernels (csrc/attn.hip) and their unfused twins (ops._SelfAttention, ops._RelPosAttention) against the
float64 restatement tests/attention_restate.py - at every edge of the 32-wide query / key tiles, on softmax rows that are flat, soft,
peaked and saturated, with NaN-filled outputs and workspaces, with split query loops (empty splits included), with padded rows that
hold large finite garbage, and under dropout with a mask rebuilt on the host.

The measure (attention_restate.slice_errors): per (utterance, head) slice and per part (out, lse, dq, dk, dv, ... each on its own),
max|kernel - float64| over the valid rows divided by the largest element of the part's magnitude version (every factor replaced by
its absolute value).  The bar of a part is max(8 * e32, 32 * 2^-24), e32 being the same measure of the same statements run in stock
float32 on the CPU: tile-ordered sums on the matrix core, v_exp_f32 for expf and the backward's re-subtraction of lse each cost about
what stock float32's own rounding costs, and that grows with the score magnitude as e32 does.  Zeros at padded rows, dq across
q_split, run-to-run equality and the `lens` equivalences are exact.  Every case prints kernel error, e32 and bar (run with -s).

Worst line per family on the MI355X: none recorded yet - this file has not been run on the device; copy them here from a `-s` run.
A float32 emulation of the fused fs2 kernels' arithmetic on the CPU (32-key tiles, log2 domain, running-max rescale, lse
re-subtracted from the recomputed scores) stays at or below 1.3 * e32 on every part of every regime of (a): out 1.7e-5 against a bar
of 1.0e-4 at `huge`, dq 1.0e-6 against 6.8e-6, lse <= 1.9e-7 against the floor 1.9e-6.
"""
import functools

import pytest
import torch

import ctts_amd  # noqa: F401
from ctts_amd import _lib
from ctts_amd import kernels as K
from ctts_amd import ops
from tests import attention_inputs as AI
from tests import attention_restate as AR

pytestmark = pytest.mark.gpu
DEV = "cuda"
LN2 = 0.6931471805599453
FLOOR = 32 * 2.0 ** -24


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def bar_of(e32):
    return max(8.0 * e32, FLOOR)


def check(tag, got, ref64_parts, mag, e32, lens, H):
    """print kernel error, e32 and bar of every part in `got`, then assert all of them"""
    e = AR.part_errors(got, ref64_parts, mag, lens, H)
    bad = []
    for n, v in e.items():
        print(f"{tag} {n}: kernel {v:.2e}  stock float32 {e32[n]:.2e}  bar {bar_of(e32[n]):.2e}")
        if not v <= bar_of(e32[n]):
            bad.append(f"{n}: {v:.3e} > {bar_of(e32[n]):.3e}")
    assert not bad, f"{tag}: " + "; ".join(bad)


def rows_beyond(t, lens):
    """[B,T,*] -> the rows >= len of every utterance, concatenated"""
    return torch.cat([t[b, min(int(n), t.shape[1]):].reshape(-1) for b, n in enumerate(lens)])


def assert_zero_rows(name, t, lens):
    z = rows_beyond(t, lens)
    assert z.numel() == 0 or bool((z == 0).all()), f"{name}: rows >= len are not exactly 0 (max |x| {z.abs().max().item()!r})"


# ---- references: computed once per input family, shared by the fused and the unfused case
@functools.lru_cache(maxsize=None)
def fs2_case(regime, B, T, H, lens, garbage=False):
    qkv, dout = AI.fs2_inputs(regime, B, T, H)
    if garbage:                                          # rows >= len hold large finite values
        pad = (torch.arange(T)[None, :] >= torch.tensor(lens)[:, None])[..., None]
        qkv, dout = torch.where(pad, qkv * 1e3, qkv), torch.where(pad, dout * 1e3, dout)
    r64 = AR.fs2_attention(qkv, lens, H, dout)
    r32 = AR.fs2_attention(qkv, lens, H, dout, dtype=torch.float32)
    e32 = AR.part_errors(AR.fs2_parts(r32), AR.fs2_parts(r64), r64.mag, lens, H)
    return qkv, dout, r64, e32


@functools.lru_cache(maxsize=None)
def rel_case(regime, B, T, H, C, p=0.0, seed_word=0, offset=0):
    qu, qv, kv, pos, dout = AI.rel_inputs(regime, B, T, H, C)
    keep = AR.attention_keep_mask(seed_word, offset, p, B, H, T) if p > 0 else None
    r64 = AR.rel_attention(qu, qv, kv, pos, H, C ** -0.5, dout, keep=keep, p_drop=p)
    r32 = AR.rel_attention(qu, qv, kv, pos, H, C ** -0.5, dout, keep=keep, p_drop=p, dtype=torch.float32)
    e32 = AR.part_errors(AR.rel_parts(r32), AR.rel_parts(r64), r64.mag, None, H)
    return (qu, qv, kv, pos, dout), keep, r64, e32


# ---- the C ABI with every output and workspace NaN-filled beforehand
def mha_abi(qkv, lens, dout, H, q_split=1):
    """-> (out, lse [log2 domain], dqkv)"""
    B, T, C3 = qkv.shape
    C = C3 // 3
    scale = (C // H) ** -0.5
    lib = _lib.load()
    out, lse = nan(B, T, C), nan(B, H, T)
    _lib.check(lib.ctts_mha_fwd(K._p(qkv), K._p(lens), K._p(out), K._p(lse), B, T, H, C, scale, K._stream()), "ctts_mha_fwd")
    Dws, dS, part, dqkv = nan(B, H, T), nan(B, H, T, T), nan(max(q_split, 1), B, T, 2 * C), nan(B, T, C3)
    _lib.check(lib.ctts_mha_bwd(K._p(qkv), K._p(lens), K._p(out), K._p(dout), K._p(lse), K._p(Dws), K._p(dS), K._p(part), K._p(dqkv),
                                B, T, H, C, scale, q_split, K._ws(qkv), K._stream()), "ctts_mha_bwd")
    return out, lse, dqkv


def relmha_abi(qu, qv, kv, pos, dout, H, scale, p=0.0, seed=None, offset=0):
    """-> (out, lse [log2 domain], dqu, dqv, dkv, dpos summed over the batch as ops._FusedRelPosAttention does)"""
    B, T, C = qu.shape
    lib = _lib.load()
    out, lse = nan(B, T, C), nan(B, H, T)
    _lib.check(lib.ctts_relmha_fwd(K._p(qu), K._p(qv), K._p(kv), K._p(pos), K._p(out), K._p(lse), B, T, H, C, scale, p, K._p(seed),
                                   offset, K._stream()), "ctts_relmha_fwd")
    Dws, dS = nan(B, H, T), nan(lib.ctts_relmha_workspace_floats(B, T, H))
    dqu, dqv, dkv, dpos_b = nan(B, T, C), nan(B, T, C), nan(B, T, 2 * C), nan(B, T, C)
    _lib.check(lib.ctts_relmha_bwd(K._p(qu), K._p(qv), K._p(kv), K._p(pos), K._p(out), K._p(dout), K._p(lse), K._p(Dws), K._p(dS),
                                   K._p(dqu), K._p(dqv), K._p(dkv), K._p(dpos_b), B, T, H, C, scale, p, K._p(seed), offset, K._stream()),
               "ctts_relmha_bwd")
    assert bool(torch.isfinite(dpos_b).all()), "dpos_b: unwritten (NaN) elements"
    return out, lse, dqu, dqv, dkv, K.colsum(dpos_b.view(B, -1)).view(T, C)


def fs2_unfused(qkv, lens, dout, H):
    ops.set_fused_attention(False)
    try:
        qg = qkv.clone().requires_grad_()
        out = ops.self_attention(qg, lens, H)
        out.backward(dout)
        return out.detach(), qg.grad
    finally:
        ops.set_fused_attention(None)


def fs2_got(out, lse, dqkv):
    C = out.shape[-1]
    got = {"out": out, "dq": dqkv[..., :C], "dk": dqkv[..., C:2 * C], "dv": dqkv[..., 2 * C:]}
    if lse is not None:
        got["lse"] = lse.double() * LN2                  # the kernel keeps log2(sum exp)
    return {n: t.cpu() for n, t in got.items()}


# ------------------------------------------------------------------------------------------------ a. fs2, every tile edge in one launch
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("regime", AI.FS2_REGIMES)
@pytest.mark.parametrize("H", AI.FS2_HEADS)
def test_fs2_tile_edges(H, regime, fused):
    """T = 97, lens 1, 2 and every tile edge -1 / 0 / +1 in one batch; d_head 32 / 64 / 128; six softmax regimes.  Fused: the C ABI
    with NaN-filled out, lse, Dws, dS, kv_part and dqkv, q_split = 1; everything comes back finite, rows >= len are exactly 0,
    two runs are bit-identical.  Unfused: ops.self_attention with the GEMM + softmax pipeline forced."""
    lens = AI.EDGE_LENS
    B, T = len(lens), AI.EDGE_T
    qkv, dout, r64, e32 = fs2_case(regime, B, T, H, lens)
    qd, dd, ld = qkv.to(DEV), dout.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    if fused:
        out, lse, dqkv = mha_abi(qd, ld, dd, H)
        for n, t in (("out", out), ("lse", lse), ("dqkv", dqkv)):
            assert bool(torch.isfinite(t).all()), f"{n}: unwritten (NaN) or non-finite elements"
        again = mha_abi(qd, ld, dd, H)
        assert all(torch.equal(a, b) for a, b in zip((out, lse, dqkv), again)), "two runs differ"
        assert_zero_rows("lse", lse.transpose(1, 2), lens)
    else:
        (out, dqkv), lse = fs2_unfused(qd, ld, dd, H), None
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all())
    assert_zero_rows("out", out, lens)
    assert_zero_rows("dqkv", dqkv, lens)
    check(f"fs2 edges {regime} H={H} {'fused' if fused else 'unfused'}", fs2_got(out, lse, dqkv), AR.fs2_parts(r64), r64.mag, e32, lens, H)


# ------------------------------------------------------------------------------------------------ b. q_split, empty splits included
@pytest.mark.parametrize("H", AI.FS2_HEADS)
def test_fs2_q_split_with_empty_splits(H):
    """K.mha_bwd with q_split 1, 2, 3, 5 on the inputs of (a), `peaked`.  Utterances of length <= 32 have one query tile, so every
    s > 1 gives them empty splits; s = 3 at four tiles (per = 2) leaves the last split empty.  dS does not depend on the split, so dq
    is bit-identical for all s; dk / dv meet the bar for every s and are bit-identical between two runs of the same s."""
    lens = AI.EDGE_LENS
    B, T, C = len(lens), AI.EDGE_T, 256
    qkv, dout, r64, e32 = fs2_case("peaked", B, T, H, lens)
    qd, dd, ld = qkv.to(DEV), dout.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    scale = (C // H) ** -0.5
    out, lse = K.mha_fwd(qd, ld, H, scale)
    dq1 = None
    for s in (1, 2, 3, 5):
        dqkv = K.mha_bwd(qd, ld, out, dd, lse, H, scale, q_split=s)
        assert bool(torch.isfinite(dqkv).all()), f"q_split={s}: non-finite gradient"
        assert torch.equal(dqkv, K.mha_bwd(qd, ld, out, dd, lse, H, scale, q_split=s)), f"q_split={s}: two runs differ"
        if dq1 is None:
            dq1 = dqkv[..., :C].clone()
        assert torch.equal(dqkv[..., :C], dq1), f"q_split={s}: dq differs from q_split=1"
        assert_zero_rows("dqkv", dqkv, lens)
        got = fs2_got(out, None, dqkv)
        check(f"fs2 q_split={s} H={H}", {n: got[n] for n in ("dq", "dk", "dv")}, AR.fs2_parts(r64), r64.mag, e32, lens, H)


# ------------------------------------------------------------------------------------------------ c. the auto rule's larger paths
@pytest.mark.parametrize("lens", [(520, 1), (513, 520)])
def test_fs2_auto_rule_q_split_and_split_k_at_their_smallest_size(lens):
    """B = 2, T = 520, H = 2, `peaked`, through ops.self_attention with the fused kernels forced.  Which path ran is pinned by
    restating the two rules and by calling K.mha_bwd directly: ops._FusedSelfAttention.backward picks q_split = 2
    (B*H*ceil(T/32) <= 2048 and T >= 256) and ctts_mha_bwd splits the dQ reduction in two (a workspace is present, T >= 512, fewer
    than 1536 output tiles); the gradient of the ops call is bit-identical to K.mha_bwd(..., q_split=2), and its dq to q_split=1.
    lens (520, 1): the second utterance has one query tile for two splits.  lens (513, 520): the last key tile is ragged by one."""
    B, T, H, C = 2, 520, 2, 256
    qkv, dout, r64, e32 = fs2_case("peaked", B, T, H, lens)
    qd, dd, ld = qkv.to(DEV), dout.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    assert ops._ATTN_Q_SPLIT == 0, "CTTS_ATTN_Q_SPLIT overrides the auto rule"
    qs = 2 if (B * H * ((T + 31) // 32) <= 2048 and T >= 256) else 1
    tiles = ((T + 63) // 64) * ((C // H + 63) // 64) * B * H
    assert qs == 2 and K._ws(qd) and tiles < 1536 and T >= 512
    ops.set_fused_attention(True)
    try:
        qg = qd.clone().requires_grad_()
        out = ops.self_attention(qg, ld, H)
        out.backward(dd)
    finally:
        ops.set_fused_attention(None)
    scale = (C // H) ** -0.5
    o2, lse = K.mha_fwd(qd, ld, H, scale)
    assert torch.equal(out.detach(), o2)
    assert torch.equal(qg.grad, K.mha_bwd(qd, ld, o2, dd, lse, H, scale, q_split=qs)), "ops did not run q_split=2"
    assert torch.equal(qg.grad[..., :C], K.mha_bwd(qd, ld, o2, dd, lse, H, scale, q_split=1)[..., :C])
    assert_zero_rows("out", o2, lens)
    assert_zero_rows("dqkv", qg.grad, lens)
    assert_zero_rows("lse", lse.transpose(1, 2), lens)
    check(f"fs2 T=520 lens={lens}", fs2_got(o2, lse, qg.grad), AR.fs2_parts(r64), r64.mag, e32, lens, H)


# ------------------------------------------------------------------------------------------------ d. length semantics
@pytest.mark.parametrize("H", AI.FS2_HEADS)
def test_fs2_length_semantics(H):
    """lens=None is lens=[T]*B, lens > T is clamped to T, and an utterance of length 0 is all zeros (out, lse, gradients: exactly 0,
    finite, from NaN-filled buffers) while its neighbours in the batch are unchanged bit for bit: padded tiles are defined as zero."""
    B, T, C = 3, 65, 256
    qkv, dout = AI.fs2_inputs("peaked", B, T, H, seed=7)
    qd, dd = qkv.to(DEV), dout.to(DEV)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=DEV)
    full = mha_abi(qd, i32([T] * B), dd, H)
    for name, lens in (("None", None), ("T+5", i32([T + 5] * B))):
        for n, a, b in zip(("out", "lse", "dqkv"), mha_abi(qd, lens, dd, H), full):
            assert torch.equal(a, b), f"lens={name}: {n} differs from lens=[T]*B"
    lens3, lens2 = [T - 3, 0, 34], [T - 3, 34]
    o3, l3, g3 = mha_abi(qd, i32(lens3), dd, H)
    for n, t in (("out", o3), ("lse", l3), ("dqkv", g3)):
        assert bool(torch.isfinite(t).all()), f"{n}: non-finite with an utterance of length 0"
        assert bool((t[1] == 0).all()), f"{n}: the utterance of length 0 is not exactly 0"
    keep = [0, 2]
    o2, l2, g2 = mha_abi(qd[keep].contiguous(), i32(lens2), dd[keep].contiguous(), H)
    for n, a, b in zip(("out", "lse", "dqkv"), (o3, l3, g3), (o2, l2, g2)):
        assert torch.equal(a[keep], b), f"{n}: an utterance of length 0 changed its neighbours"
    r64 = AR.fs2_attention(qkv, lens3, H, dout)
    r32 = AR.fs2_attention(qkv, lens3, H, dout, dtype=torch.float32)
    e32 = AR.part_errors(AR.fs2_parts(r32), AR.fs2_parts(r64), r64.mag, lens3, H)
    check(f"fs2 lens={lens3} H={H}", fs2_got(o3, l3, g3), AR.fs2_parts(r64), r64.mag, e32, lens3, H)


# ------------------------------------------------------------------------------------------------ e. finite garbage at padded rows
@pytest.mark.parametrize("fused", [True, False])
def test_fs2_padded_rows_hold_finite_garbage(fused):
    """(a) with `peaked`, H = 2, rows >= len of qkv and dout multiplied by 1e3: a leak of 1e-8 of a padded row into a valid one
    shows.  The float64 reference ignores those rows by construction; the gradient at them is exactly 0."""
    lens, H = AI.EDGE_LENS, 2
    B, T = len(lens), AI.EDGE_T
    qkv, dout, r64, e32 = fs2_case("peaked", B, T, H, lens, garbage=True)
    clean = fs2_case("peaked", B, T, H, lens)[2]
    assert all(torch.equal(getattr(r64, n), getattr(clean, n)) for n in AR.FS2_PARTS), "the reference itself reads padded rows"
    qd, dd, ld = qkv.to(DEV), dout.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    if fused:
        out, lse, dqkv = mha_abi(qd, ld, dd, H)
        assert_zero_rows("lse", lse.transpose(1, 2), lens)
    else:
        (out, dqkv), lse = fs2_unfused(qd, ld, dd, H), None
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all())
    assert_zero_rows("out", out, lens)
    assert_zero_rows("dqkv", dqkv, lens)
    check(f"fs2 garbage {'fused' if fused else 'unfused'}", fs2_got(out, lse, dqkv), AR.fs2_parts(r64), r64.mag, e32, lens, H)


# ------------------------------------------------------------------------------------------------ f. relative-position attention
def rel_run(ts, H, scale, fused, p=0.0):
    """-> {part: tensor on the CPU}; fused: C ABI on NaN-filled buffers, unfused: ops.relpos_attention"""
    qu, qv, kv, pos, dout = [t.to(DEV) for t in ts]
    C = qu.shape[-1]
    drop = K.DropCtx(DEV, seed=77) if p > 0 else None
    if fused:
        seed, off = (drop.seed, drop.next_offset()) if drop is not None else (None, 0)
        out, lse, dqu, dqv, dkv, dpos = relmha_abi(qu, qv, kv, pos, dout, H, scale, p, seed, off)
        lse = lse.double() * LN2
    else:
        ops.set_fused_attention(False)
        try:
            tg = [t.clone().requires_grad_() for t in (qu, qv, kv, pos)]
            out = ops.relpos_attention(*tg, H, scale, p_drop=p, drop=drop)
            out.backward(dout)
            out, lse = out.detach(), None
            dqu, dqv, dkv, dpos = [t.grad for t in tg]
        finally:
            ops.set_fused_attention(None)
    got = {"out": out, "dqu": dqu, "dqv": dqv, "dk": dkv[..., :C], "dv": dkv[..., C:], "dpos": dpos}
    if lse is not None:
        got["lse"] = lse
    for n, t in got.items():
        assert bool(torch.isfinite(t).all()), f"{n}: unwritten (NaN) or non-finite elements"
    return {n: t.cpu() for n, t in got.items()}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("regime", AI.REL_REGIMES)
@pytest.mark.parametrize("H,C", AI.REL_HC)
def test_rel_tile_edges(H, C, regime, fused):
    """T = 1, 2 and every tile edge -1 / 0 / +1 up to 97, B = 2, d_head 32 / 64 / 128, the model's scale C^-0.5.  position_peaked lets
    the position band decide every row: a wrong band row or the wrong side of x = T moves the peak."""
    scale = C ** -0.5
    failures = []
    for T in AI.REL_T:
        ts, _, r64, e32 = rel_case(regime, 2, T, H, C)
        got = rel_run(ts, H, scale, fused)
        try:
            check(f"rel {regime} T={T} H={H} C={C} {'fused' if fused else 'unfused'}", got, AR.rel_parts(r64), r64.mag, e32, None, H)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ g. dropout against float64
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("regime", ["soft", "content_peaked"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("T", [33, 65])
def test_rel_dropout_against_float64(T, p, regime, fused):
    """Values and all four gradients under dropout against float64 with the keep mask rebuilt on the host from DropCtx's seed word
    and the offset the call consumed (the first of a fresh context: 1).  First the mask itself: K.relpos_softmax_fwd returns P and
    the dropped Pd, and Pd != 0 must equal the restated mask wherever P > 0 - a hash mismatch is reported as such."""
    B, H, C = 2, 8, 256
    dh, scale = C // H, C ** -0.5
    word = int(K.DropCtx(DEV, seed=77).seed.item()) & 0xFFFFFFFFFFFFFFFF
    ts, keep, r64, e32 = rel_case(regime, B, T, H, C, p, word, 1)
    qu, qv, kv, pos, _ = [t.to(DEV) for t in ts]
    drop = K.DropCtx(DEV, seed=77)
    sS = (H * T * T, T * T)
    S, PS = torch.empty(B, H, T, T, device=DEV), torch.empty(B, H, T, T, device=DEV)
    K.gemm(qu, kv, S, T, T, dh, C, 2 * C, T, True, True, nb0=B, nb1=H, sA=(T * C, dh), sB=(T * 2 * C, dh), sC=sS)
    K.gemm(qv, pos, PS, T, T, dh, C, C, T, True, True, nb0=B, nb1=H, sA=(T * C, dh), sB=(0, dh), sC=sS)
    Pd = K.relpos_softmax_fwd(S, PS, T, scale, p, drop.seed, drop.next_offset(), want_dropped=True)      # S <- P
    seen = S.cpu() > 0                                   # a probability that underflowed to 0 does not show its mask bit
    wrong = int(((Pd.cpu() != 0) != keep)[seen].sum())
    assert wrong == 0, f"the restated keep mask differs from the kernel's in {wrong} of {seen.numel()} elements"
    got = rel_run(ts, H, scale, fused, p)
    check(f"rel dropout {regime} T={T} p={p} {'fused' if fused else 'unfused'}", got, AR.rel_parts(r64), r64.mag, e32, None, H)
