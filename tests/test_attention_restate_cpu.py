"""Keeps the float64 attention oracle (tests/attention_restate.py) honest without a GPU: its closed-form gradients against autograd on
the textbook formula, its shift against the element rule in the header of csrc/attn.hip, its dropout mask's elementary properties, and
the conditioning of every input family of tests/test_attention_gpu.py (stock float32 stays below 5e-5 in the test's own measure)."""
import pytest
import torch

from tests import attention_inputs as AI
from tests import attention_restate as AR

CAP32 = 5e-5


def rnd(*shape, seed):
    return AI.base(*shape, seed=seed).double()


def test_fs2_closed_form_gradients_equal_autograd():
    B, T, C, H = 3, 37, 64, 2
    dh = C // H
    lens = torch.tensor([37, 18, 30])
    qkv, dout = rnd(B, T, 3 * C, seed=1) * 3, rnd(B, T, C, seed=2)
    leaf = qkv.clone().requires_grad_()
    q, k, v = (t.reshape(B, T, H, dh).transpose(1, 2) for t in leaf.split(C, dim=-1))
    pad = torch.arange(T)[None, :] >= lens[:, None]
    s = ((q * dh ** -0.5) @ k.transpose(-1, -2)).masked_fill(pad[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, C) * (~pad)[..., None]
    o.backward(dout)
    lse = torch.logsumexp(s, -1).detach() * (~pad)[:, None, :]
    r = AR.fs2_attention(qkv, lens, H, dout)
    g = leaf.grad
    for name, got, ref in (("out", r.out, o.detach()), ("lse", r.lse, lse), ("dq", r.dq, g[..., :C]), ("dk", r.dk, g[..., C:2 * C]),
                           ("dv", r.dv, g[..., 2 * C:])):
        err = (got - ref).abs().max().item()
        assert err <= 1e-12, (name, err)
    for name, m in r.mag.items():                       # a magnitude version bounds its tensor, element by element
        assert (m + 1e-15 >= getattr(r, name).abs()).all(), name


@pytest.mark.parametrize("p_drop", [0.0, 0.3])
def test_rel_closed_form_gradients_equal_autograd(p_drop):
    B, T, C, H = 3, 37, 64, 2
    dh = C // H
    scale = C ** -0.5 * 4
    ts = [rnd(B, T, C, seed=3) * 2, rnd(B, T, C, seed=4) * 2, rnd(B, T, 2 * C, seed=5), rnd(T, C, seed=6)]
    dout = rnd(B, T, C, seed=7)
    keep = AR.attention_keep_mask(1234567, 3, p_drop, B, H, T) if p_drop > 0 else None
    qu, qv, kv, pos = leaves = [t.clone().requires_grad_() for t in ts]
    q1 = qu.view(B, T, H, dh).transpose(1, 2)
    q2 = qv.view(B, T, H, dh).transpose(1, 2)
    k = kv[..., :C].reshape(B, T, H, dh).permute(0, 2, 1, 3)
    v = kv[..., C:].reshape(B, T, H, dh).permute(0, 2, 1, 3)
    p = pos.view(T, H, dh).permute(1, 2, 0)[None]
    ps = q2 @ p
    padded = torch.cat([ps.new_zeros(B, H, T, 1), ps], dim=-1).view(B, H, T + 1, T)
    score = (q1 @ k.transpose(2, 3) + padded[:, :, 1:].reshape(B, H, T, T)) * scale
    attn = torch.softmax(score, -1)
    if keep is not None:
        attn = attn * keep.double() / (1 - p_drop)
    o = (attn @ v).transpose(1, 2).reshape(B, T, C)
    o.backward(dout)
    r = AR.rel_attention(*ts, H, scale, dout, keep=keep, p_drop=p_drop)
    for name, got, ref in (("out", r.out, o.detach()), ("lse", r.lse, torch.logsumexp(score, -1).detach()), ("dqu", r.dqu, qu.grad),
                           ("dqv", r.dqv, qv.grad), ("dkv", r.dkv, kv.grad), ("dpos", r.dpos, pos.grad)):
        err = (got - ref).abs().max().item()
        assert err <= 1e-12, (name, err)
    parts = AR.rel_parts(r)
    for name, m in r.mag.items():
        assert (m + 1e-15 >= parts[name].abs()).all(), name


@pytest.mark.parametrize("T", [1, 2, 5, 33])
def test_shift_equals_the_kernels_element_rule(T):
    """x = j - i + T - 1:  x <= T-1: QV[i] . pos[x],  x == T: 0,  x >= T+1: QV[i+1] . pos[x-T-1]"""
    dh = 4
    qv, pos = rnd(T, dh, seed=10 + T), rnd(T, dh, seed=20 + T)
    got = AR.rel_shift((qv @ pos.t())[None, None])[0, 0]
    want = torch.zeros(T, T, dtype=torch.float64)
    for i in range(T):
        for j in range(T):
            x = j - i + T - 1
            if x <= T - 1:
                want[i, j] = qv[i] @ pos[x]
            elif x >= T + 1:
                want[i, j] = qv[i + 1] @ pos[x - T - 1]
    assert torch.equal(got, want) or (got - want).abs().max().item() <= 1e-15
    g = rnd(T, T, seed=30 + T)[None, None]              # rel_unshift is the adjoint: <shift(a), g> = <a, unshift(g)>
    a = rnd(T, T, seed=40 + T)[None, None]
    assert abs(((AR.rel_shift(a) * g).sum() - (a * AR.rel_unshift(g)).sum()).item()) <= 1e-12


def test_keep_mask_share_purity_and_offsets():
    B, H, T = 2, 8, 113                                  # 204,304 elements
    assert B * H * T * T >= 2e5
    for p in (0.1, 0.5):
        m = AR.attention_keep_mask(0x123456789ABCDEF, 4, p, B, H, T)
        assert m.shape == (B, H, T, T) and m.dtype == torch.bool
        assert abs(m.double().mean().item() - (1 - p)) < 0.01
        assert torch.equal(m, AR.attention_keep_mask(0x123456789ABCDEF, 4, p, B, H, T))
        assert not torch.equal(m, AR.attention_keep_mask(0x123456789ABCDEF, 5, p, B, H, T))
        assert not torch.equal(m, AR.attention_keep_mask(0x123456789ABCDEE, 4, p, B, H, T))
    assert AR.attention_keep_mask(1, 1, 0.0, 1, 1, 9).all()
    # the 32-bit finaliser itself, by hand: mix32(0) = 0 and one worked value
    assert int(AR.ctts_mix32(0)) == 0
    x = 1
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16      # noqa: E702
    assert int(AR.ctts_mix32(1)) == x


def test_slice_errors_is_per_slice_and_per_part():
    B, T, H, C = 2, 5, 2, 4
    ref = torch.ones(B, T, C, dtype=torch.float64)
    mag = torch.ones(B, T, C, dtype=torch.float64)
    mag[1, :, 2:] = 100.0                                # slice (1, head 1) is a hundred times larger
    got = ref.clone()
    got[0, 0, 0] += 1e-3
    got[1, 1, 3] += 1e-3
    got[1, 4, 0] += 7.0                                  # a padded row of utterance 1: ignored
    tab = AR.slice_error_table(got, ref, mag, [5, 4], H)
    assert tab.shape == (B, H)
    assert abs(tab[0, 0].item() - 1e-3) < 1e-12 and tab[0, 1].item() == 0 and tab[1, 0].item() == 0
    assert abs(tab[1, 1].item() - 1e-5) < 1e-12
    assert abs(AR.slice_errors(got, ref, mag, [5, 4], H) - 1e-3) < 1e-12
    zero = torch.zeros(B, H, T, dtype=torch.float64)     # exact parts: a magnitude of 0 admits only the exact value
    assert AR.slice_errors(zero, zero, zero, None, H, rows_last=True) == 0.0
    assert AR.slice_errors(zero + 1e-30, zero, zero, None, H, rows_last=True) == float("inf")
    assert AR.slice_errors(zero * float("nan"), zero, zero + 1, None, H, rows_last=True) == float("inf")


# ---- conditioning of the GPU test's inputs: stock float32 on the same statements stays below 5e-5 in the same measure
def _fs2_e32(qkv, dout, lens, H):
    r64, r32 = AR.fs2_attention(qkv, lens, H, dout), AR.fs2_attention(qkv, lens, H, dout, dtype=torch.float32)
    return AR.part_errors(AR.fs2_parts(r32), AR.fs2_parts(r64), r64.mag, lens, H)


@pytest.mark.parametrize("H", AI.FS2_HEADS)
@pytest.mark.parametrize("regime", AI.FS2_REGIMES)
def test_fs2_edge_inputs_are_well_conditioned(regime, H):
    B, T = len(AI.EDGE_LENS), AI.EDGE_T
    qkv, dout = AI.fs2_inputs(regime, B, T, H)
    e = _fs2_e32(qkv, dout, AI.EDGE_LENS, H)
    print(f"fs2 {regime} H={H}: " + "  ".join(f"{n} {v:.1e}" for n, v in e.items()))
    assert max(e.values()) < CAP32, e


@pytest.mark.parametrize("lens", [(520, 1), (513, 520)])
def test_fs2_long_inputs_are_well_conditioned(lens):
    qkv, dout = AI.fs2_inputs("peaked", 2, 520, 2)
    e = _fs2_e32(qkv, dout, lens, 2)
    print(f"fs2 peaked T=520 lens={lens}: " + "  ".join(f"{n} {v:.1e}" for n, v in e.items()))
    assert max(e.values()) < CAP32, e


@pytest.mark.parametrize("H,C", AI.REL_HC)
@pytest.mark.parametrize("regime", AI.REL_REGIMES)
def test_rel_inputs_are_well_conditioned(regime, H, C):
    worst = {}
    for T in AI.REL_T:
        qu, qv, kv, pos, dout = AI.rel_inputs(regime, 2, T, H, C)
        r64 = AR.rel_attention(qu, qv, kv, pos, H, C ** -0.5, dout)
        r32 = AR.rel_attention(qu, qv, kv, pos, H, C ** -0.5, dout, dtype=torch.float32)
        e = AR.part_errors(AR.rel_parts(r32), AR.rel_parts(r64), r64.mag, None, H)
        worst = {n: max(v, worst.get(n, 0.0)) for n, v in e.items()}
    print(f"rel {regime} H={H} C={C}: " + "  ".join(f"{n} {v:.1e}" for n, v in worst.items()))
    assert max(worst.values()) < CAP32, worst


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("regime", ["soft", "content_peaked"])
def test_rel_dropout_inputs_are_well_conditioned(regime, p):
    H, C = 8, 256
    for T in (33, 65):
        qu, qv, kv, pos, dout = AI.rel_inputs(regime, 2, T, H, C)
        keep = AR.attention_keep_mask(77, 1, p, 2, H, T)
        r64 = AR.rel_attention(qu, qv, kv, pos, H, C ** -0.5, dout, keep=keep, p_drop=p)
        r32 = AR.rel_attention(qu, qv, kv, pos, H, C ** -0.5, dout, keep=keep, p_drop=p, dtype=torch.float32)
        e = AR.part_errors(AR.rel_parts(r32), AR.rel_parts(r64), r64.mag, None, H)
        print(f"rel dropout {regime} p={p} T={T}: " + "  ".join(f"{n} {v:.1e}" for n, v in e.items()))
        assert max(e.values()) < CAP32, e
