"""CPU: tests/seq_restate64.py (the float64 oracle of tests/test_seq_kernels_gpu.py) against the stock torch ops it restates -
torch.nn.GRU and autograd through it, F.conv1d(groups=C), F.glu, F.unfold / F.conv2d - and the sanity of its float32 run, the
yardstick of the GPU tests: within 1e-5 of the float64 run by the GPU tests' own measures (rows against their RMS, sums against the
L2 norm of their summands)."""
import pytest
import torch
import torch.nn.functional as F

from tests import seq_restate64 as S

TOL = 1e-12
D, F32 = torch.float64, torch.float32
TINY = 1e-300


def near(a, b, name):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= TOL * max(1.0, b.abs().max().item() if b.numel() else 1.0), f"{name}: {err:.3e}"


def rows_err(got, ref, dim=-1):
    got, ref = got.double(), ref.double()
    return ((got - ref).abs().amax(dim) / ref.pow(2).mean(dim).sqrt().clamp_min(TINY)).max().item()


def scaled_err(got, ref, scale):
    return ((got.double() - ref.double()).abs() / scale.double().clamp_min(TINY)).max().item()


# ------------------------------------------------------------------------------------------------ GRU
def stock_gru(H, bi, seed):
    torch.manual_seed(seed)
    return torch.nn.GRU(3 * H, H, batch_first=True, bidirectional=bi).double()


def stock_params(ref, sfx=""):
    return [getattr(ref, n + sfx).detach() for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]


@pytest.mark.parametrize("T", [1, 11])
@pytest.mark.parametrize("H", [16, 32])
@pytest.mark.parametrize("bi", [False, True], ids=["uni", "bi"])
def test_gru_restatement_and_its_bptt_equal_stock_float64(bi, H, T):
    B, ndir = 3, 2 if bi else 1
    ref = stock_gru(H, bi, 10 * H + T)
    g = torch.Generator().manual_seed(T)
    x = torch.randn(B, T, 3 * H, generator=g, dtype=D)
    dout = torch.randn(B, T, ndir, H, generator=g, dtype=D)
    prm = [stock_params(ref)] + ([stock_params(ref, "_reverse")] if bi else [])
    gi = torch.stack([x @ p[0].t() + p[2] for p in prm], 2)                          # [B,T,ndir,3H]
    whh, bhh = torch.stack([p[1] for p in prm]), torch.stack([p[3] for p in prm])
    r = S.gru(gi, whh, bhh, 2 if bi else 0, dout)
    xl = x.clone().requires_grad_()
    mem, _ = ref(xl)
    mem.backward(dout.reshape(B, T, ndir * H))
    near(r["out"].reshape(B, T, ndir * H), mem, "out")
    # dgi against autograd: dx = sum_d dgi_d W_ih_d, dW_ih_d = dgi_d^T x, db_ih_d = column sums of dgi_d
    near(sum(r["dgi"][:, :, d] @ prm[d][0] for d in range(ndir)), xl.grad, "dx from dgi")
    for d, sfx in enumerate(["", "_reverse"][:ndir]):
        near(torch.einsum("bti,btj->ij", r["dgi"][:, :, d], x), getattr(ref, "weight_ih_l0" + sfx).grad, "dW_ih" + sfx)
        near(r["dgi"][:, :, d].sum((0, 1)), getattr(ref, "bias_ih_l0" + sfx).grad, "db_ih" + sfx)
        near(r["dwhh"][d], getattr(ref, "weight_hh_l0" + sfx).grad, "dW_hh" + sfx)
        near(r["dbhh"][d], getattr(ref, "bias_hh_l0" + sfx).grad, "db_hh" + sfx)
    # what the restatement says about its own by-products
    H3 = 3 * H
    near(r["gates"][..., 3 * H:], torch.einsum("btdj,dij->btdi", r["hprev"], whh[:, 2 * H:]) + bhh[:, 2 * H:], "ghn = W_hn h + b_hn")
    assert (r["hprev"][:, 0, 0] == 0).all() and (not bi or (r["hprev"][:, T - 1, 1] == 0).all())
    if T > 1:
        assert torch.equal(r["hprev"][:, 1:, 0], r["out"][:, :-1, 0])
        if bi:
            assert torch.equal(r["hprev"][:, :-1, 1], r["out"][:, 1:, 1])
    assert r["dgh"].shape == (B, T, ndir, H3)
    assert torch.equal(r["dgh"][..., :2 * H], r["dgi"][..., :2 * H])
    near(r["dgh"][..., 2 * H:], r["dgi"][..., 2 * H:] * r["gates"][..., :H], "dgh_n = dgi_n * r")
    assert (r["dwhh_norm"] >= r["dwhh"].abs() / (B * T) ** 0.5 - 1e-12).all() and (r["dbhh_norm"] >= r["dbhh"].abs() / (B * T) ** 0.5 - 1e-12).all()


@pytest.mark.parametrize("H,T", [(16, 1), (32, 11)])
def test_gru_reverse_masks_equal_flipped_forward_runs(H, T):
    """rev_mask = 1 (one reversed sequence) and the three-direction mask 0b101: each reversed direction is the forward run of the
    time-flipped input, flipped back - values and every gradient"""
    for ndir, mask in ((1, 1), (3, 0b101)):
        i = S.gru_inputs(3, T, H, ndir, seed=mask)
        r = S.gru(i["gi"], i["whh"], i["bhh"], mask, i["dout"])
        for d in range(ndir):
            rev = (mask >> d) & 1
            fl = (lambda t: t.flip(1)) if rev else (lambda t: t)
            one = S.gru(fl(i["gi"][:, :, d:d + 1]), i["whh"][d:d + 1], i["bhh"][d:d + 1], 0, fl(i["dout"][:, :, d:d + 1]))
            for q in ("out", "gates", "hprev", "dgi", "dgh"):
                near(r[q][:, :, d], fl(one[q])[:, :, 0], f"mask {mask} dir {d} {q}")
            for q in ("dwhh", "dbhh", "dwhh_norm", "dbhh_norm"):
                near(r[q][d], one[q][0], f"mask {mask} dir {d} {q}")
        distinct = r["out"][:, :, 0] if ndir == 1 else r["out"][:, :, 0] - r["out"][:, :, 2]
        assert distinct.abs().max() > 1e-3


# ------------------------------------------------------------------------------------------------ depthwise conv
@pytest.mark.parametrize("K", [1, 3, 31])
@pytest.mark.parametrize("T", [1, 5, 14, 40])
def test_dwconv_restatement_equals_stock_float64(T, K):
    """T = 1, 5 and 14 are shorter than K / 2 for K = 31 (every output sees both paddings)"""
    B, C = 2, 8
    i = S.dw_inputs(B, T, C, K, seed=1)
    r = S.dwconv(i["x"], i["w"], i["dy"])
    x, w = i["x"].double().requires_grad_(), i["w"].double().requires_grad_()
    y = F.conv1d(x.transpose(1, 2), w.view(C, 1, K), padding=(K - 1) // 2, groups=C).transpose(1, 2)
    y.backward(i["dy"].double())
    near(r["y"], y, "y")
    near(r["dx"], x.grad, "dx")
    near(r["dw"], w.grad, "dw")
    # the norms are those of the summands: K = 1 has one summand per output
    if K == 1:
        near(r["y_norm"], y.abs(), "y_norm")
        near(r["dx_norm"], x.grad.abs(), "dx_norm")
    assert (r["y_norm"] * K ** 0.5 >= r["y"].abs() - 1e-12).all() and (r["dx_norm"] * K ** 0.5 >= r["dx"].abs() - 1e-12).all()
    assert (r["dw_norm"] * (B * T) ** 0.5 >= r["dw"].abs() - 1e-12).all()
    near(r["dw_norm"][:, (K - 1) // 2], (i["dy"].double() * i["x"].double()).pow(2).sum((0, 1)).sqrt(), "dw_norm of the centre tap")


# ------------------------------------------------------------------------------------------------ GLU, relattn_split
@pytest.mark.parametrize("rows,C", [(1, 4), (9, 12)])
def test_glu_restatement_equals_stock_float64(rows, C):
    i = S.glu_inputs(rows, C, seed=2)
    r = S.glu(i["a"], i["dout"])
    a = i["a"].double().requires_grad_()
    out = F.glu(a, -1)
    out.backward(i["dout"].double())
    near(r["out"], out, "out")
    near(r["da"], a.grad, "da")
    assert i["a"][:, C:].abs().max() == (100.0 if rows * C >= 3 else 30.0)


def test_relattn_split_restatement_is_two_adds_and_a_copy_and_its_adjoint():
    i = S.split_inputs(7, 8, seed=3)
    qkv, u, v = [i[k].double().requires_grad_() for k in ("qkv", "u", "v")]
    qu, qv, kv = S.relattn_split(qkv, u, v)
    near(qu, qkv[:, :8] + u, "qu")
    near(qv, qkv[:, :8] + v, "qv")
    assert torch.equal(kv, qkv[:, 8:])
    ((qu * i["dqu"]).sum() + (qv * i["dqv"]).sum() + (kv * i["dkv"]).sum()).backward()
    near(S.relattn_split_bwd(i["dqu"], i["dqv"], i["dkv"]), qkv.grad, "dqkv")
    q32 = S.relattn_split(i["qkv"], i["u"], i["v"], F32)
    assert q32[0].dtype == F32 and torch.equal(q32[0], i["qkv"][:, :8] + i["u"]) and torch.equal(q32[2], i["qkv"][:, 8:])


# ------------------------------------------------------------------------------------------------ Conv2d patches
PATCH_SHAPES = [(1, 1, 1, 4), (2, 1, 2, 4), (2, 2, 3, 8), (1, 3, 4, 8), (2, 2, 5, 4), (1, 3, 80, 4)]


@pytest.mark.parametrize("B,T,W,C", PATCH_SHAPES)
def test_im2col_equals_unfold_and_its_product_equals_conv2d(B, T, W, C):
    i = S.patch_inputs(B, T, W, C, seed=4)
    x = i["x"].double()
    Wo = (W - 1) // 2 + 1
    col = S.im2col_3x3s2(x)
    assert col.shape == (B * T * Wo, 9 * C)
    # F.unfold on [B,C,T,W]: columns ordered (c, kh, kw), blocks (t, wo)
    u = F.unfold(x.permute(0, 3, 1, 2), (3, 3), padding=(1, 1), stride=(1, 2))          # [B, C*9, T*Wo]
    u = u.view(B, C, 9, T * Wo).permute(0, 3, 2, 1).reshape(B * T * Wo, 9 * C)
    assert torch.equal(col, u)
    assert torch.equal(S.im2col_3x3s2(i["x"]).double(), col), "the float32 gather is the float64 gather"
    Cout = 5
    w = torch.randn(Cout, C, 3, 3, generator=torch.Generator().manual_seed(W), dtype=D)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, stride=(1, 2), padding=(1, 1)).permute(0, 2, 3, 1)
    near((col @ w.permute(0, 2, 3, 1).reshape(Cout, 9 * C).t()).view(B, T, Wo, Cout), y, "im2col @ w")


@pytest.mark.parametrize("B,T,W,C", PATCH_SHAPES)
def test_col2im_is_the_adjoint_of_im2col(B, T, W, C):
    i = S.patch_inputs(B, T, W, C, seed=5)
    x, dcol = i["x"].double().requires_grad_(), i["dcol"].double()
    S.im2col_3x3s2(x).backward(dcol)
    dx, norm = S.col2im_3x3s2(dcol, B, T, W, C)
    near(dx, x.grad, "col2im against autograd")
    lhs, rhs = (S.im2col_3x3s2(x.detach()) * dcol).sum(), (x.detach() * dx).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), "<im2col(x), d> == <x, col2im(d)>"
    # the number of patch entries an input element collects: at most 6, and the norm is that of exactly those entries
    ones, cnt_norm = S.col2im_3x3s2(torch.ones_like(dcol), B, T, W, C)
    assert ones.max() <= 6 and torch.equal(cnt_norm, ones.sqrt())
    if W % 2 == 0:
        assert ones[:, :, W - 1].max() <= 3, "the last column of an even W is read through kw = 2 only"
    assert (norm * 6 ** 0.5 >= dx.abs() - 1e-12).all()


# ------------------------------------------------------------------------------------------------ the float32 yardstick
YARD = 1e-5


def test_float32_runs_are_within_1e_5_of_float64_by_the_gpu_measures():
    i = S.gru_inputs(3, 25, 32, 2, seed=6)
    r64, r32 = [S.gru(i["gi"], i["whh"], i["bhh"], 2, i["dout"], dtype=t) for t in (D, F32)]
    assert r32["out"].dtype == F32
    for q in ("out", "gates", "dgi", "dgh"):
        blocks = 4 if q == "gates" else 1
        for a, b in zip(r32[q].chunk(blocks, -1), r64[q].chunk(blocks, -1)):
            assert rows_err(a, b) <= YARD, q
    assert scaled_err(r32["dwhh"], r64["dwhh"], r64["dwhh_norm"]) <= YARD and scaled_err(r32["dbhh"], r64["dbhh"], r64["dbhh_norm"]) <= YARD
    i = S.dw_inputs(2, 70, 16, 31, seed=7)
    r64, r32 = [S.dwconv(i["x"], i["w"], i["dy"], dtype=t) for t in (D, F32)]
    for q in ("y", "dx", "dw"):
        assert scaled_err(r32[q], r64[q], r64[q + "_norm"]) <= YARD, q
    i = S.glu_inputs(9, 12, seed=8)
    r64, r32 = [S.glu(i["a"], i["dout"], dtype=t) for t in (D, F32)]
    x, d = i["a"][:, :12].double(), i["dout"].double()
    assert scaled_err(r32["out"], r64["out"], x.abs()) <= YARD
    assert scaled_err(r32["da"][:, :12], r64["da"][:, :12], d.abs()) <= YARD
    assert scaled_err(r32["da"][:, 12:], r64["da"][:, 12:], (d * x).abs()) <= YARD
    i = S.patch_inputs(2, 3, 6, 8, seed=9)
    (d64, n64), (d32, _) = [S.col2im_3x3s2(i["dcol"], 2, 3, 6, 8, dtype=t) for t in (D, F32)]
    assert scaled_err(d32, d64, n64) <= YARD
    i = S.split_inputs(5, 8, seed=10)
    for a, b in zip(S.relattn_split(i["qkv"], i["u"], i["v"], F32), S.relattn_split(i["qkv"], i["u"], i["v"])):
        assert scaled_err(a, b, b.abs()) <= YARD
    assert scaled_err(S.relattn_split_bwd(i["dqu"], i["dqv"], i["dkv"], F32), S.relattn_split_bwd(i["dqu"], i["dqv"], i["dkv"]),
                      torch.cat([i["dqu"].abs() + i["dqv"].abs(), i["dkv"].abs()], -1)) <= YARD


def test_seeded_inputs_are_reproducible_and_differ_per_utterance_direction_and_channel():
    a, b = S.gru_inputs(3, 9, 16, 2), S.gru_inputs(3, 9, 16, 2)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["gi"][0], a["gi"][1]) and not torch.equal(a["gi"][:, :, 0], a["gi"][:, :, 1])
    assert not torch.equal(a["whh"][0], a["whh"][1])
    s = S.gru_inputs(3, 9, 16, 2, gi_scale=5.0, spike=200.0)["gi"]
    assert (s == 200.0).any() and (s == -200.0).any() and s.abs().max() == 200.0
    d = S.dw_inputs(2, 9, 8, 3)
    assert not torch.equal(d["x"][0], d["x"][1]) and not torch.equal(d["w"][0], d["w"][1]) and d["old"].abs().min() > 0
