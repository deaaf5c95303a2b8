"""CPU: tests/norm_restate64.py (the float64 oracle of tests/test_norm_kernels_gpu.py) against the stock torch ops it restates, the
determinism of the seeded inputs the GPU tests draw, and the conditioning of the BatchNorm offset inputs: stock float32 keeps rstd to
1e-7 at every offset, so a kernel that misses its bar there has a precision bug of its own."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_restate64 as N

TOL = 1e-12


def near(a, b, name):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= TOL * max(1.0, b.abs().max().item() if b.numel() else 1.0), f"{name}: {err:.3e}"


@pytest.mark.parametrize("rows,C,eps", [(1, 4, 1e-5), (37, 252, 1e-12), (67, 1024, 1e-5)])
def test_layernorm_restatement_equals_stock_float64(rows, C, eps):
    i = N.ln_inputs(rows, C, seed=1)
    r = N.layer_norm_grads(i["x"], i["gamma"], i["beta"], eps, i["dy"], rowscale=i["rowscale"], dres=i["dres"])
    x, g, b = [i[k].double().requires_grad_() for k in ("x", "gamma", "beta")]
    y = F.layer_norm(x, (C,), g, b, eps) * i["rowscale"].double()[:, None]
    y.backward(i["dy"].double())
    near(r["y"], y, "y")
    near(r["dx"], x.grad + i["dres"].double(), "dx")
    near(r["dgamma"], g.grad, "dgamma")
    near(r["dbeta"], b.grad, "dbeta")
    near(r["sg"].sum(0), g.grad, "summands of dgamma")
    near(r["sb"].sum(0), b.grad, "summands of dbeta")
    near(r["mean"], x.mean(-1), "mean")
    near(r["rstd"], 1 / torch.sqrt(x.var(-1, unbiased=False) + eps), "rstd")
    dead = i["rowscale"] == 0
    assert (r["y"][dead] == 0).all() and (dead.any() or rows == 1)


def test_layernorm_restatement_dropout_is_the_mask_times_the_scale():
    i = N.ln_inputs(9, 8, seed=2)
    keep = torch.rand(9, 8, generator=torch.Generator().manual_seed(0)) < 0.5
    r = N.layer_norm_grads(i["x"], i["gamma"], i["beta"], 1e-5, i["dy"], keep=keep, p=0.5)
    x, g, b = [i[k].double().requires_grad_() for k in ("x", "gamma", "beta")]
    y = F.layer_norm(x, (8,), g, b, 1e-5) * keep.double() * 2.0
    y.backward(i["dy"].double())
    near(r["y"], y, "y")
    near(r["dx"], x.grad, "dx")
    near(r["dbeta"], b.grad, "dbeta")


@pytest.mark.parametrize("act", N.ACTS)
@pytest.mark.parametrize("rows,C", [(2, 8), (150, 36)])
def test_batchnorm_restatement_equals_stock_float64(rows, C, act):
    i = N.bn_inputs(rows, C, offset=3.0, seed=3)
    fn = {"none": lambda t: t, "tanh": torch.tanh, "swish": F.silu}[act]
    r = N.batch_norm_grads(i["x"], i["gamma"], i["beta"], 1e-5, i["dy"], act=act, running_mean=i["running_mean"],
                           running_var=i["running_var"], momentum=0.1)
    x, g, b = [i[k].double().requires_grad_() for k in ("x", "gamma", "beta")]
    rm, rv = i["running_mean"].double().clone(), i["running_var"].double().clone()
    y = fn(F.batch_norm(x, rm, rv, g, b, True, 0.1, 1e-5))
    y.backward(i["dy"].double())
    for k, ref in (("y", y), ("dx", x.grad), ("dgamma", g.grad), ("dbeta", b.grad), ("running_mean", rm), ("running_var", rv)):
        near(r[k], ref, k)
    near(r["sg"].sum(0), g.grad, "summands of dgamma")
    near(r["sb"].sum(0), b.grad, "summands of dbeta")
    assert r["num_batches_inc"] == 1
    bn = torch.nn.BatchNorm1d(C).double()                                            # the module, for num_batches_tracked
    bn(i["x"].double())
    assert int(bn.num_batches_tracked) == r["num_batches_inc"]
    mean, var, rstd = N.batch_stats(i["x"], 1e-5)
    near(mean, r["mean"], "batch_stats mean")
    near(rstd, r["rstd"], "batch_stats rstd")
    # eval mode: the running statistics, no update
    e = N.batch_norm_grads(i["x"], i["gamma"], i["beta"], 1e-5, i["dy"], act=act, training=False, running_mean=rm, running_var=rv)
    x2, g2, b2 = [i[k].double().requires_grad_() for k in ("x", "gamma", "beta")]
    ye = fn(F.batch_norm(x2, rm, rv, g2, b2, False, 0.1, 1e-5))
    ye.backward(i["dy"].double())
    near(e["y"], ye, "eval y")
    near(e["dx"], x2.grad, "eval dx")
    near(e["dgamma"], g2.grad, "eval dgamma")
    assert "running_mean" not in e


def test_batchnorm_restatement_single_row_keeps_the_biased_variance_in_the_running_update():
    m, v, inc = N.running_update(torch.tensor([2.0]), torch.tensor([0.0]), 1, torch.tensor([1.0]), torch.tensor([1.0]), 0.1)
    assert abs(float(m) - 1.1) < 1e-15 and abs(float(v) - 0.9) < 1e-15 and inc == 1


@pytest.mark.parametrize("T,lens", [(1, [1, 1]), (5, [3, 5]), (65, [1, 33])])
def test_square_softmax_restatement_equals_masked_fill_softmax(T, lens):
    S, dP = N.score_inputs((2, 2, T, T), seed=4)
    P, dS = N.softmax_grads(lambda s: N.softmax_square(s, lens), S, dP)
    Sl = S.double().requires_grad_()
    kmask = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]                  # [nb0, T]
    ref = torch.softmax(Sl.masked_fill(kmask[:, None, None, :], float("-inf")), -1).masked_fill(kmask[:, None, :, None], 0.0)
    ref.backward(dP.double())
    near(P, ref, "P")
    near(dS, Sl.grad, "dS")
    for b, L in enumerate(lens):
        assert (P[b, :, L:] == 0).all() and (P[b, :, :, L:] == 0).all() and (dS[b, :, L:] == 0).all() and (dS[b, :, :, L:] == 0).all()


@pytest.mark.parametrize("Tq,Tk,klens,qlens", [(1, 1, [1, 0], None), (5, 32, [0, 1, 32], [5, 5, 0]), (7, 9, [9, 4, 1], [0, 7, 3])])
def test_rect_softmax_restatement_equals_masked_fill_softmax(Tq, Tk, klens, qlens):
    nb = len(klens)
    S, dP = N.score_inputs((nb, Tq, Tk), seed=5)
    P, dS = N.softmax_grads(lambda s: N.softmax_rect(s, klens, qlens), S, dP)
    Sl = S.double().requires_grad_()
    kmask = torch.arange(Tk)[None, :] >= torch.tensor(klens)[:, None]
    dead = (torch.arange(Tq)[None, :] >= torch.tensor(qlens if qlens is not None else [Tq] * nb)[:, None]) | (torch.tensor(klens) == 0)[:, None]
    safe = Sl.masked_fill(kmask[:, None, :], float("-inf")).masked_fill(dead[:, :, None], 0.0)       # dead rows: any finite row, zeroed below
    ref = torch.softmax(safe, -1).masked_fill(dead[:, :, None] | kmask[:, None, :], 0.0)
    ref.backward(dP.double())
    near(P, ref, "P")
    near(dS, Sl.grad, "dS")
    assert (P[dead] == 0).all() and (dS[dead] == 0).all()
    assert (P.masked_select(kmask[:, None, :].expand_as(P)) == 0).all()


@pytest.mark.parametrize("T", [1, 2, 5, 64])
def test_rel_shift_restatement_equals_the_padded_view_and_its_adjoint(T):
    nb = 3
    PS, dS = N.score_inputs((nb, T, T), seed=6)
    ps = PS.double().requires_grad_()
    padded = torch.cat([ps.new_zeros(1, nb, T, 1), ps[None]], dim=-1).view(1, nb, T + 1, T)          # as in test_relpos_attention_fwd_bwd
    shifted = padded[:, :, 1:].reshape(nb, T, T)
    assert torch.equal(N.rel_shift(PS.double()), shifted.detach())
    shifted.backward(dS.double())
    assert torch.equal(N.rel_shift_adjoint(dS.double()), ps.grad)
    assert torch.equal(N.rel_shift_adjoint(dS).double(), ps.grad)                                    # a gather: exact in float32 too
    # index form quoted by the kernel: shifted.flat[i * T + j] = padded.flat[i * T + j + T]
    flat = torch.cat([PS.new_zeros(nb, T, 1), PS], -1).reshape(nb, -1)
    assert torch.equal(N.rel_shift(PS).reshape(nb, -1), flat[:, T:])


@pytest.mark.parametrize("T,scale", [(1, 1.0), (9, 0.25), (65, 1.0)])
def test_relpos_softmax_restatement_equals_stock_softmax(T, scale):
    S, dP = N.score_inputs((3, T, T), seed=7)
    PS, _ = N.score_inputs((3, T, T), seed=8)
    Sl, Pl = S.double().requires_grad_(), PS.double().requires_grad_()
    P, _ = N.relpos_softmax(Sl, Pl, scale)
    P.backward(dP.double())
    S2, P2 = S.double().requires_grad_(), PS.double().requires_grad_()
    padded = torch.cat([P2.new_zeros(3, T, 1), P2], dim=-1).view(3, T + 1, T)
    ref = torch.softmax((S2 + padded[:, 1:].reshape(3, T, T)) * scale, -1)
    ref.backward(dP.double())
    near(P, ref, "P")
    near(Sl.grad, S2.grad, "dS")
    near(Pl.grad, P2.grad, "dPS")
    keep = torch.rand(3, T, T, generator=torch.Generator().manual_seed(1)) < 0.8
    _, Pd = N.relpos_softmax(S, PS, scale, keep=keep, p=0.2)
    near(Pd, ref.detach() * keep.double() / 0.8, "Pd")


def test_input_generators_are_deterministic_and_distinct():
    for fn, args in ((N.bn_inputs, (150, 80, 30.0)), (N.ln_inputs, (67, 516)), (N.ln_inputs, (8, 4, 0, 1000.0))):
        a, b = fn(*args), fn(*args)
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (fn.__name__, k)
            assert a[k].dtype == torch.float32
    a, b = N.score_inputs((3, 65, 65), seed=2), N.score_inputs((3, 65, 65), seed=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(N.score_inputs((3, 65, 65), seed=3)[0], a[0])
    assert not torch.equal(N.bn_inputs(150, 80, 0.0)["x"], N.bn_inputs(150, 80, 0.0, seed=1)["x"])
    i = N.bn_inputs(150, 80, 300.0)
    m = i["x"].mean(0)
    assert (m[0::2] > 299).all() and (m[1::2] < -299).all()
    r = N.ln_inputs(257, 256)["rowscale"]
    assert (r == 0).any() and (r == 1).any() and ((r != 0) & (r != 1)).any()
    assert (N.ln_inputs(8, 4, 0, 1000.0)["x"].mean(-1).abs() > 990).all()


@pytest.mark.parametrize("rows,C", [(150, 80), (4096, 32)])
@pytest.mark.parametrize("offset", [0.0, 3.0, 30.0, 300.0])
def test_offset_inputs_are_well_conditioned_for_stock_float32(rows, C, offset):
    """The batch variance of the offset inputs in stock float32 (two-pass: the restatement in float32, and torch.var_mean), carried to
    rstd in float64 so that only the statistics' own error shows, against float64: <= 1e-7 relative at every offset (measured about
    3e-8).  The offsets themselves cost float32 nothing - only a one-pass E[x^2] - mean^2 loses digits on them."""
    x = N.bn_inputs(rows, C, offset)["x"]
    _, _, r64 = N.batch_stats(x, 1e-5)
    _, v32r, _ = N.batch_stats(x, 1e-5, dtype=torch.float32)
    v32, _ = torch.var_mean(x, 0, unbiased=False)
    for name, v in (("restatement", v32r), ("var_mean", v32)):
        assert v.dtype == torch.float32
        err = ((1.0 / torch.sqrt(v.double() + 1e-5) - r64).abs() / r64).max().item()
        print(f"offset {offset:g} [{rows}, {C}] {name}: float32 statistics, rstd rel err {err:.2e}")
        assert err <= 1e-7, (name, err)
