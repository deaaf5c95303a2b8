"""CPU: tests/glue_restate64.py (the oracle of tests/test_glue_kernels_gpu.py) against the stock torch ops it restates -
repeat_interleave / cumsum / searchsorted for the length regulator, F.embedding and autograd through it, autograd through the unfused
positional-embedding and GEMM-epilogue expressions with the dropout mask given - and the sanity of its float32 run, the yardstick of
the GPU tests.

The second half shows that the GPU tests can fail: for every edge they aim at, a deliberately wrong MODEL (never a wrong kernel) gives
a different answer than the restatement on the very inputs the GPU tests use - the carry dropped at element 64, a lower-bound search,
the crop applied at the phoneme, the padding row not zeroed, the dropout index of the float4 instead of the element, a folded column
sum that adds copy j into channel j % k, and the partials of count - 1 stripes."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import glue_restate64 as S
from tests.gemm_restate64 import act, keep_mask

TOL = 1e-12
D, F32 = torch.float64, torch.float32
TINY = 1e-300
SEED_U64 = 0x1234_5678_9ABC_DEF1
OFFSET = 3


def near(a, b, name):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= TOL * max(1.0, b.abs().max().item() if b.numel() else 1.0), f"{name}: {err:.3e}"


def scaled_err(got, ref, scale):
    return ((got.double() - ref.double()).abs() / scale.double().clamp_min(TINY)).max().item()


# ================================================================================================ length regulator
def one_duration(v, round_mode):
    """the per-element rule of include/ctts.h, one Python number at a time"""
    if isinstance(v, float):
        if v != v or v <= 0:
            return 0
        if v == float("inf"):
            return S.DUR_CAP
        return min(int(round(v) if round_mode else math.trunc(v)), S.DUR_CAP)       # Python's round: half to even
    return min(max(v, 0), S.DUR_CAP)


def stock_lr_index(d, Tm):
    """d int64 [B,Ts] (already by the duration rule) -> mel2ph, mel_len by cumsum + searchsorted(right=True)"""
    cum = d.cumsum(1)
    t = torch.arange(Tm).expand(d.shape[0], Tm).contiguous()
    m = torch.searchsorted(cum, t, right=True) + 1
    return torch.where(t < cum[:, -1:], m, torch.zeros_like(m)).to(torch.int32), cum[:, -1]


LR_INPUTS = [(Ts, kind) for Ts in S.LR_TS for kind in ("int64", "int64big", "float32")]


def lr_input(Ts, kind):
    return S.lr_float_durations(Ts) if kind == "float32" else S.lr_int_durations(Ts, big=kind == "int64big")


@pytest.mark.parametrize("Ts,kind", LR_INPUTS)
def test_duration_rule_and_index_match_stock_torch(Ts, kind):
    dur, u8 = lr_input(Ts, kind), S.lr_pad(Ts)
    for rm in (0, 1):
        for pad in (None, u8, u8.bool()):
            d = S.durations(dur, pad, rm)
            want = torch.tensor([[0 if (pad is not None and pad[b, i]) else one_duration(dur[b, i].item(), rm) for i in range(Ts)]
                                 for b in range(S.LR_B)])
            assert torch.equal(d, want)
            for Tm in S.lr_tm_set(int(d[0].sum())):
                mel2ph, mel_len, cum = S.lr_index(dur, Tm, pad, rm)
                sm, sl = stock_lr_index(d, Tm)
                assert torch.equal(mel2ph, sm) and torch.equal(mel_len, sl) and torch.equal(cum.long(), d.cumsum(1).clamp(max=S.INT32_MAX))
                for b in range(S.LR_B):
                    if int(mel_len[b]) < 10000:              # repeat_interleave materialises the frames: small totals only
                        frames = torch.repeat_interleave(torch.arange(1, Ts + 1), d[b])[:Tm]
                        assert torch.equal(mel2ph[b].long(), F.pad(frames, (0, Tm - len(frames))))


def test_float_rows_hold_every_special_value():
    d = S.lr_float_durations(65)
    flat = d.flatten().tolist()
    for v in (0.5, 1.5, 2.5, -3.0, 2.0e9, float("inf")):
        assert v in flat
    assert any(v != v for v in flat) and any(v == 0 and math.copysign(1, v) < 0 for v in flat)
    assert S.durations(torch.tensor([[0.5, 1.5, 2.5, -3.0, -0.0, float("nan"), 2.0e9, float("inf"), 3.9]]), None, 1).tolist() == \
        [[0, 2, 2, 0, 0, 0, S.DUR_CAP, S.DUR_CAP, 4]]
    assert S.durations(torch.tensor([[0.5, 1.5, 2.5, 3.9]]), None, 0).tolist() == [[0, 1, 2, 3]]


def test_overflow_row_keeps_the_exact_total():
    for dur in S.lr_overflow_durations():
        mel2ph, mel_len, cum = S.lr_index(dur, 300)
        assert (mel2ph == 4).all() and mel_len.tolist() == [4_000_000_000]
        assert cum[0, :3].tolist() == [0, 0, 0] and (cum[0, 3:64] == S.DUR_CAP).all() and int(cum[0, 64]) == S.INT32_MAX
        # what a scan in 32-bit integers makes of it: the total wraps to a negative number and every frame reads as padding
        wrapped = (int(mel_len[0]) + 2 ** 31) % 2 ** 32 - 2 ** 31
        assert wrapped < 0


def gather_case(B, Ts, C, Tm, dur):
    x = S.randn(B, Ts, C, seed=Tm)
    mel2ph, _, cum = S.lr_index(dur, Tm)
    return x, mel2ph, cum


@pytest.mark.parametrize("B,Ts,C", S.GATHER_FWD_CASES + [(2, S.GATHER_BWD_TS, 4)])
def test_gather_and_its_gradient_match_autograd(B, Ts, C):
    dur = S.gather_durations(B, Ts, seed=1)
    for Tm in S.gather_fwd_tms(dur):
        x, mel2ph, cum = gather_case(B, Ts, C, Tm, dur)
        xs = x.double().requires_grad_()
        stock = torch.gather(F.pad(xs, (0, 0, 1, 0)), 1, mel2ph.long()[..., None].expand(B, Tm, C))
        near(S.lr_gather(x, mel2ph), stock, "lr_gather")
        assert torch.equal(S.lr_gather(x, mel2ph, F32), stock.detach().float())
        dy = S.randn(B, Tm, C, seed=C)
        stock.backward(dy.double())
        dx, norm = S.lr_gather_grad(dy, cum)
        near(dx, xs.grad, "lr_gather_grad")
        assert ((norm == 0).all(-1) == ((dur == 0) | (F.pad(cum, (1, 0))[:, :-1] >= Tm))).all()
        assert scaled_err(S.lr_gather_grad(dy, cum, F32)[0], dx, norm) < 1e-5


@pytest.mark.parametrize("T", S.POSITIONS_T)
def test_positions_match_cumsum(T):
    s = S.positions_int_input(T)
    nz = (s != 0).long()
    assert torch.equal(S.positions(s).long(), nz.cumsum(1) * nz)
    x = S.positions_float_input(T)
    nz = x[..., 0].ne(0).long()
    assert torch.equal(S.positions(x, x.shape[2]).long(), nz.cumsum(1) * nz)
    assert (x[..., 1:] != 0).all() and (S.positions(x, x.shape[2])[2] == 0).all()
    if T > 4:
        assert torch.isnan(x[1, :, 0]).any() and (S.positions(x, x.shape[2])[1][torch.isnan(x[1, :, 0])] > 0).all()


# ================================================================================================ embedding
@pytest.mark.parametrize("n", [1, 65, 4096])
def test_embedding_and_its_gradient_match_autograd(n):
    V, C = S.EMB_V, 8
    ids, dy, old, w = S.embedding_ids(n, V), S.randn(n, C, seed=1), S.randn(V, C, seed=2), S.randn(V, C, seed=3)
    ok = (ids >= 0) & (ids < V)
    out = S.embedding(ids, w)
    near(out[ok], F.embedding(ids[ok], w.double()), "embedding")
    assert (out[~ok] == 0).all()
    for pad in (-1, 0, V - 1, V):
        ws = w.double().requires_grad_()
        F.embedding(ids[ok], ws, padding_idx=pad if 0 <= pad < V else None).backward(dy[ok].double())
        dw, norm = S.embedding_grad(ids, dy, V, pad)
        near(dw, ws.grad, f"embedding_grad padding_idx {pad}")
        acc, accn = S.embedding_grad(ids, dy, V, pad, old)
        near(acc, old.double() + ws.grad, "embedding_grad accumulate")
        near(accn, norm + old.abs(), "embedding_grad accumulate norm")
        assert scaled_err(S.embedding_grad(ids, dy, V, pad, dtype=F32)[0], dw, norm) < 1e-5
    assert not (ids == V // 2).any()
    if n >= 8:
        assert (ids == -1).any() and (ids == V).any() and (ids == V + 3).any()


# ================================================================================================ posembed, epilogue
def test_drop_scale_is_the_restated_mask():
    rows, C, p = S.DROP_ROWS, 11, 0.1
    d = S.drop_scale(SEED_U64, OFFSET, p, rows, C)
    keep = keep_mask(SEED_U64, OFFSET, p, np.arange(rows * C).reshape(rows, C))
    assert torch.equal(d != 0, keep) and 0.02 < 1 - keep.double().mean() < 0.25
    assert set(d.unique().tolist()) == {0.0, float(np.float32(1) / np.float32(0.9))}
    assert (S.drop_scale(SEED_U64, OFFSET, 0.0, rows, C) == 1).all()


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_posembed_matches_autograd_through_the_unfused_expression(p):
    rows, C = 16, 64
    x, dy, rs, table = S.randn(rows, C, seed=4), S.randn(rows, C, seed=6), S.rowscale_input(rows), S.randn(9, C, seed=7)
    pos = torch.randint(0, 9, (rows,), generator=torch.Generator().manual_seed(rows)).to(torch.int32)
    drop = S.drop_scale(SEED_U64, OFFSET, p, rows, C)
    xs, alpha = x.double().requires_grad_(), torch.tensor([0.7], dtype=D, requires_grad=True)
    y = rs.double()[:, None] * (drop * (xs + alpha * F.embedding(pos.long(), table.double())))
    y.backward(dy.double())
    near(S.posembed(x, pos, table, alpha.detach(), rs, drop), y, "posembed")
    dx, dalpha, norm = S.posembed_grad(dy, pos, table, rs, drop)
    near(dx, xs.grad, "posembed dx")
    near(dalpha, alpha.grad, "posembed dalpha")
    old = torch.tensor([0.37])
    near(S.posembed_grad(dy, pos, table, rs, drop, old)[1], alpha.grad + old.double(), "posembed dalpha accumulate")
    near(S.posembed(x, pos, table, None, None, drop), drop * (x.double() + table.double()[pos.long()]), "posembed without alpha / rowscale")
    assert scaled_err(S.posembed_grad(dy, pos, table, rs, drop.float(), dtype=F32)[1], dalpha, norm) < 1e-5


@pytest.mark.parametrize("code", [0, 1, 2, 3, 4])
def test_epilogue_backward_matches_autograd_through_the_unfused_expression(code):
    rows, C, p = 33, 11, 0.1
    dy, z, rs, old = S.randn(rows, C, seed=8), S.act_z(rows, C), S.rowscale_input(rows), S.randn(C, seed=9)
    drop = S.drop_scale(SEED_U64, OFFSET, p, rows, C)
    zs, bias, R = z.double().requires_grad_(), torch.zeros(C, dtype=D, requires_grad=True), torch.zeros(rows, C, dtype=D, requires_grad=True)
    if code == 1:
        assert (z != 0).sum() == z.numel() - 2                # ReLU'(0) = 0 here and in autograd alike; the exact zeros are the two planted
    y = rs.double()[:, None] * (R + drop * act(zs + 0.5 * bias, code))
    y.backward(dy.double())
    r = S.epilogue_bwd(dy, rs, z, code, drop, 0.5, None)
    near(r["gm"], R.grad, "epilogue gm")
    near(r["dz"], zs.grad, "epilogue dz")
    near(r["dbias"], bias.grad, "epilogue dbias")
    near(S.epilogue_bwd(dy, rs, z, code, drop, 0.5, old)["dbias"], old.double() + bias.grad, "epilogue dbias accumulate")
    near(r["dbias_norm"], 0.5 * r["dz"].pow(2).sum(0).sqrt(), "epilogue dbias norm")
    a, scale = S.act_dropout_bwd(dy, z, code, drop)
    zs2 = z.double().requires_grad_()
    (drop * act(zs2, code)).backward(dy.double())
    near(a, zs2.grad, "act_dropout_bwd")
    near(scale, (dy.double() * drop).abs(), "act_dropout_bwd scale")
    near(S.rowscale_dropout(dy, rs, drop), rs.double()[:, None] * drop * dy.double(), "rowscale_dropout")
    r32 = S.epilogue_bwd(dy, rs, z, code, drop.float(), 0.5, None, dtype=F32)
    assert scaled_err(r32["dz"], r["dz"], r["dz_scale"]) < 1e-5 and scaled_err(r32["dbias"], r["dbias"], r["dbias_norm"]) < 1e-5


def test_act_z_holds_the_special_values():
    z = S.act_z(600, 200).flatten().tolist()
    for v in (0.0, 1e-3, -1e-3, 20.0, -20.0):
        assert float(np.float32(v)) in z


def test_column_sums_and_partial_sums_match_stock_torch():
    rows, C = 96, 5
    x, w, old = S.randn(rows, C + 7, seed=14), S.randn(rows, seed=10), S.randn(C, seed=11)
    xv = x[:, 3:3 + C]
    out, norm = S.colsum(xv, -0.5, old)
    near(out, old.double() - 0.5 * xv.double().sum(0), "colsum")
    near(norm, 0.5 * xv.double().norm(dim=0) + old.abs(), "colsum norm")
    near(S.colsum(xv)[0], xv.double().sum(0), "colsum plain")
    near(S.weighted_colsum(xv, w, 2.0, old)[0], old.double() + 2.0 * torch.einsum("r,rc->c", w.double(), xv.double()), "weighted_colsum")
    for n, count, stride, _ in S.psum_tasks()[:6]:
        src, dst = S.randn(count * stride, seed=20), S.randn(n, seed=50)
        got, pn = S.partial_sums(dst, src, count, stride, n, -0.5)
        near(got, dst.double() - 0.5 * src.double().view(count, stride)[:, :n].sum(0), "partial_sums")
        near(pn, 0.5 * src.double().view(count, stride)[:, :n].norm(dim=0) + dst.abs(), "partial_sums norm")
        assert scaled_err(S.partial_sums(dst, src, count, stride, n, -0.5, F32)[0], got, pn) < 1e-5


def test_fold_factor_and_task_list_reach_the_paths_they_name():
    assert [S.colsum_fold(64 * 17, C) for C in S.COLSUM_NARROW_C] == [64, 32, 16, 8, 2]
    assert all(S.colsum_fold(64 * 17 + 1, C) == 1 for C in S.COLSUM_NARROW_C)
    assert [S.colsum_fold(96, C) for C in S.COLSUM_NARROW_C] == [32, 32, 16, 8, 2]
    assert [S.colsum_fold(1000, C) for C in S.COLSUM_NARROW_C] == [8, 8, 8, 8, 2]
    assert S.colsum_fold(64 * 17, 5, ld=12) == 1 and S.colsum_fold(64 * 17, 64) == 1
    tasks = S.psum_tasks()
    assert len(tasks) == 25 and {t[1] for t in tasks} == {1, 7, 8, 9} and tasks[0][0] > 8192
    assert any(t[3] == 1 and t[0] % 4 for t in tasks) and any(t[2] % 4 for t in tasks)
    assert [r * c // 4 for r, c in S.DALPHA_SHAPES] == [1, 256, 4480]
    B, Ts, C, Tm = S.GATHER_FWD_LOOP
    assert B * Tm * (C // 4) > 2048 * 256


# ================================================================================================ the inputs discriminate
def chunked_prefix(d, chunk=64):
    """WRONG: the inclusive scan restarts at every 64th element (the carry between the chunks is dropped)"""
    return torch.cat([c.cumsum(1) for c in d.split(chunk, 1)], 1)


def index_from_prefix(prefix, Tm, lower_bound=False):
    t = torch.arange(Tm)
    count = ((prefix[:, None, :] < t[None, :, None]) if lower_bound else (prefix[:, None, :] <= t[None, :, None])).sum(-1)
    total = prefix[:, -1:].clamp(max=Tm)
    return torch.where(t[None, :] < total, 1 + count, torch.zeros_like(count)).to(torch.int32)


@pytest.mark.parametrize("Ts,kind", LR_INPUTS)
def test_lr_inputs_tell_a_dropped_carry_and_a_lower_bound_search(Ts, kind):
    dur = lr_input(Ts, kind)
    for rm in (0, 1):
        d = S.durations(dur, None, rm)
        total = int(d[0].sum())
        right = {Tm: S.lr_index(dur, Tm, None, rm) for Tm in S.lr_tm_set(total)}
        for Tm, (mel2ph, mel_len, cum) in right.items():
            assert torch.equal(index_from_prefix(d.cumsum(1), Tm), mel2ph)
        # lower bound: the first frame of a phoneme goes to the one before - visible once Tm reaches past the first phoneme of row 0
        # (3 frames at most) and a second phoneme exists
        if Ts > 1:
            assert all(not torch.equal(index_from_prefix(d.cumsum(1), Tm, lower_bound=True), r[0]) for Tm, r in right.items() if Tm > 3)
            assert sum(Tm > 3 for Tm in right) >= 4
        if Ts > 64:
            wrong = chunked_prefix(d)
            assert not torch.equal(wrong.clamp(max=S.INT32_MAX).to(torch.int32), right[600][2]), "cum"
            assert not torch.equal(wrong[:, -1], right[600][1]), "mel_len"
            assert not torch.equal(index_from_prefix(wrong, 600), right[600][0]), "mel2ph"
            # row 2 (int64): the single non-zero at element 64 is the one entry a lost carry cannot hide behind
            if kind == "int64":
                assert (d[2, :64] == 0).all() and d[2, 64] == 5


@pytest.mark.parametrize("T", [65, 130])
def test_position_inputs_tell_a_dropped_carry(T):
    for src, stride in ((S.positions_int_input(T), 1), (S.positions_float_input(T), 3)):
        nz = ((src if src.dim() == 2 else src[..., 0]) != 0).long()
        wrong = chunked_prefix(nz) * nz
        right = S.positions(src, stride).long()
        assert not torch.equal(wrong, right)
        if T > 66:                   # at T = 65 row 0 is zero at element 64, the only one behind the first chunk: the other rows tell
            assert (wrong[0] != right[0]).any(), "the row with zeros at the chunk boundaries tells them apart"


@pytest.mark.parametrize("C", [4, 256])
def test_gather_gradient_inputs_tell_a_crop_at_the_phoneme(C):
    B, Ts = 2, S.GATHER_BWD_TS
    dur = S.gather_durations(B, Ts, seed=1)
    Tm = S.gather_fwd_tms(dur)[0]
    cum = S.lr_index(dur, Tm)[2]
    dy = S.randn(B, Tm, C, seed=C)
    dx, norm = S.lr_gather_grad(dy, cum)
    start = F.pad(cum, (1, 0))[:, :-1]
    cut = (start < Tm) & (cum > Tm)
    assert cut[0].sum() == 1, "Tm cuts one run of row 0 in the middle"
    for whole in (False, True):
        # WRONG: a phoneme whose run crosses Tm is dropped whole / summed whole
        wrong = dx.clone()
        for b, i in cut.nonzero().tolist():
            wrong[b, i] = 0 if not whole else dy.double()[b, int(start[b, i]):].sum(0) * 2
        assert scaled_err(wrong, dx, norm) > 1e-3
    long = S.gather_durations(B, Ts, seed=1, long_run=300)
    assert (long == 300).sum() == 1 and (long == 0).any()


@pytest.mark.parametrize("n", [63, 64, 65, 4095, 16385])
def test_embedding_inputs_tell_a_padding_row_that_is_not_zeroed(n):
    V, C = S.EMB_V, 4
    ids, dy = S.embedding_ids(n, V), S.randn(n, C, seed=1)
    for pad in (0, V - 1):
        assert (ids == pad).any()
        dw, norm = S.embedding_grad(ids, dy, V, pad)
        wrong, _ = S.embedding_grad(ids, dy, V, -1)             # WRONG: the padding row gets its gradient
        assert (dw[pad] == 0).all() and (wrong[pad] != 0).any()
    # an id outside [0, V) that is clamped into the table instead of dropped would show in rows 0 and V - 1
    clamped, _ = S.embedding_grad(ids.clamp(0, V - 1), dy, V, -1)
    dw, norm = S.embedding_grad(ids, dy, V, -1)
    assert scaled_err(clamped, dw, norm.clamp_min(1e-30)) > 1e-3


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("C", [4, 64, 200])
def test_dropout_inputs_tell_the_float4_index_from_the_element_index(C, p):
    rows = S.DROP_ROWS
    right = S.drop_scale(SEED_U64, OFFSET, p, rows, C) != 0
    r, c = np.divmod(np.arange(rows * C).reshape(rows, C), C)
    wrong = keep_mask(SEED_U64, OFFSET, p, r * (C // 4) + c // 4)            # WRONG: row * (C / 4) + c4
    assert not torch.equal(right, wrong)
    x = S.randn(rows, C, seed=4)
    assert not torch.equal(S.rowscale_dropout(x, None, right.float(), F32), S.rowscale_dropout(x, None, wrong.float(), F32))


def folded_colsum(x, k, wrong=False):
    """the folded view of ctts_colsum: [rows, C] read as [rows / k, k * C], the k copies of a channel added at the end"""
    rows, C = x.shape
    view = x.double().reshape(rows // k, k * C).sum(0)
    out = torch.zeros(C, dtype=D)
    for j in range(k * C):
        ch = j % k if wrong else j % C                         # WRONG: copy j goes to channel j % k
        if ch < C:
            out[ch] += view[j]
    return out


@pytest.mark.parametrize("rows", S.COLSUM_ROWS)
@pytest.mark.parametrize("C", S.COLSUM_NARROW_C)
def test_narrow_colsum_inputs_tell_a_fold_into_the_wrong_channel(C, rows):
    x = S.randn(rows, C, seed=12)
    k = S.colsum_fold(rows, C)
    ref, norm = S.colsum(x)
    near(folded_colsum(x, k), ref, "the folded view sums to the plain column sums")
    if k > 1 and k != C:
        assert scaled_err(folded_colsum(x, k, wrong=True), ref, norm) > 1e-3


def test_partial_sum_inputs_tell_a_missing_stripe():
    for t, (n, count, stride, _) in enumerate(S.psum_tasks()):
        src, dst, alpha = S.randn(count * stride, seed=20 + t), S.randn(n, seed=50 + t), (1.0, -0.5, 2.0)[t % 3]
        right, norm = S.partial_sums(dst, src, count, stride, n, alpha)
        wrong, _ = S.partial_sums(dst, src, count - 1, stride, n, alpha)     # WRONG: count - 1 stripes
        assert scaled_err(wrong, right, norm) > 1e-3, t
    x = S.randn(64 * 17, 65, seed=30)
    right, norm = S.colsum(x)
    assert scaled_err(S.colsum(x[:64 * 16])[0], right, norm) > 1e-3          # the 17th stripe of 64 rows left out
