"""GPU: the normalisation and softmax kernels - LayerNorm, BatchNorm1d and the masked square softmax (csrc/norm.hip), the rectangular
softmax (csrc/prosody.hip) and the relative-position softmax and shift (csrc/conformer.hip) - against the float64 restatement
tests/norm_restate64.py, at the sizes where their template instantiations, folds, grids and code paths change.

Error measure (never the tensor's global maximum): per row for LayerNorm and the softmaxes, per channel for BatchNorm,
max |got - ref64| over the row / channel divided by that row's / channel's reference RMS; a reference row of zeros must be met exactly.
Quantities that are one number per row / channel use the scale of what they are made of: mean, dgamma, dbeta and the BatchNorm mean
are sums, measured against the L2 norm of their float64 summands (a sum that cancels to nearly 0 keeps a meaningful scale); rstd and
running_var are positive, measured relative to themselves; running_mean against (1 - m) |old| + m |batch mean|.

Bar of every quantity: max(8 x the error of the same restatement run in float32 on the CPU (same input, same measure), 4 * 2^-23).
The factor 8 covers a different summation order plus the hardware __expf and rsqrtf; the floor covers the final float rounding, the
float add of eps and rsqrtf.  Every comparison prints `kernel err / stock float32 err / bar` (run with -s).

Measured on the MI355X, worst case per quantity (kernel error / stock float32 error / bar; 791 comparisons, none above 0.47 of its bar):
  BatchNorm train step   mean 5.3e-8 / 5.3e-8 / 4.8e-7   rstd 6.0e-8 / 7.6e-8 / 6.1e-7   y 3.6e-7 / 2.6e-7 / 2.0e-6   dx 2.3e-6 / 1.0e-6 / 8.2e-6
                         dgamma 4.3e-7 / 3.7e-7 / 3.0e-6   dbeta 2.3e-7 / 1.3e-7 / 1.0e-6   running_mean 1.2e-7 / 1.2e-7 / 9.5e-7
                         running_var 1.0e-7 / 8.8e-8 / 7.0e-7   eval y 1.0e-6 / 6.4e-7 / 5.1e-6   eval dbeta 3.6e-6 / 1.2e-6 / 9.6e-6
  BatchNorm offset sweep rstd 8.6e-8 / 9.8e-8 / 7.8e-7   y 4.0e-7 / 4.8e-7 / 3.9e-6   dx 5.9e-7 / 6.1e-7 / 4.9e-6   mean 2.4e-6 / 6.7e-6 / 5.4e-5
                         (float32 per-thread sums, as before the fix: rstd 4.8e-5 at offset 30 and 6.1e-3 at 300 on [150, 80], 9.0e-6 and
                         9.1e-4 on [4096, 32], against bars of about 1e-6: those four cases fail)
  BatchNorm dropout      y 1.7e-7 / 1.9e-7 / 1.5e-6   dx 8.6e-7 / 7.4e-7 / 5.9e-6   dgamma 1.3e-7 / 1.7e-7 / 1.3e-6   dbeta 2.7e-7 / 2.5e-7 / 2.0e-6
  LayerNorm              mean 5.2e-7 / 3.7e-7 / 3.0e-6   rstd 6.6e-8 / 5.2e-8 / 4.8e-7   y 6.7e-7 / 6.0e-7 / 4.8e-6   dx 2.2e-7 / 1.1e-7 / 8.6e-7
                         dgamma 1.7e-7 / 1.2e-7 / 9.7e-7   dbeta 3.4e-7 / 2.7e-7 / 2.1e-6   no workspace: dx 5.9e-7 / 6.9e-7 / 5.5e-6
  LayerNorm, mean 1000   y 1.0e-4 / 1.5e-4 / 1.2e-3   dx 1.2e-5 / 1.2e-5 / 9.3e-5   dgamma 1.2e-4 / 1.6e-4 / 1.3e-3   rstd 1.2e-7 / 1.0e-7 / 8.2e-7
  LayerNorm dropout      y 2.8e-7 / 2.9e-7 / 2.3e-6   dx 8.3e-7 / 7.9e-7 / 6.3e-6   dgamma 3.9e-7 / 3.5e-7 / 2.8e-6   dbeta 3.0e-7 / 3.0e-7 / 2.4e-6
  square softmax         P 1.1e-5 / 6.4e-6 / 5.1e-5 (T 1025, streaming path)   dS 1.6e-5 / 4.2e-6 / 3.3e-5 (T 65: 3.8 x stock, the largest ratio)
                         row sums within 3.6e-7 of 1 (bound 1.5e-5 at L = 1025)
  rectangular softmax    P 6.0e-7 / 3.6e-7 / 2.9e-6   dS 2.8e-6 / 1.7e-6 / 1.3e-5
  relpos softmax         P 1.3e-6 / 8.5e-7 / 6.8e-6   dS 1.3e-5 / 8.5e-6 / 6.8e-5   with dropout: Pd 1.4e-6 / 1.2e-6 / 9.7e-6   dS 1.3e-6 / 8.9e-7 / 7.1e-6
The per-row measure divides by the row's RMS, not its maximum: a softmax row of L keys reads sqrt(L) larger than its error relative to the
peak, for the kernel and for stock float32 alike.
"""
import functools
import math

import pytest
import torch

import ctts_amd  # noqa: F401
from ctts_amd import _lib
from ctts_amd import kernels as K
from ctts_amd import ops
from tests import norm_restate64 as N

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 4 * 2.0 ** -23
FACTOR = 8.0
TINY = 1e-300
ACT = {"none": K.ACT_NONE, "tanh": K.ACT_TANH, "swish": K.ACT_SWISH}
D, F32 = torch.float64, torch.float32


def dev(t):
    return None if t is None else t.to(DEV)


def c64(t):
    return t.detach().double().cpu()


def err_rows(got, ref64, dim):
    """worst over the rows (all dims but `dim`) of max |got - ref64| / RMS(ref64), both taken along `dim`"""
    got, ref64 = c64(got), c64(ref64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    if ref64.numel() == 0:
        return 0.0
    d = (got - ref64).abs().amax(dim)
    rms = ref64.pow(2).mean(dim).sqrt()
    return (d / rms.clamp_min(TINY)).max().item()


def err_scaled(got, ref64, scale):
    """worst |got - ref64| / scale, element for element (scale 0: the element must be met exactly)"""
    got, ref64 = c64(got), c64(ref64)
    assert got.shape == ref64.shape == scale.shape, (got.shape, ref64.shape, scale.shape)
    return ((got - ref64).abs() / scale.double().clamp_min(TINY)).max().item() if got.numel() else 0.0


def judge(name, e, e32):
    bar = max(FACTOR * e32, FLOOR)
    print(f"{name}: kernel err {e:.2e}  stock float32 {e32:.2e}  bar {bar:.2e}")
    assert math.isfinite(e) and e <= bar, f"{name}: kernel err {e:.3e} > bar {bar:.3e} (stock float32 {e32:.3e})"


def check_rows(name, got, r64, r32, dim):
    assert torch.isfinite(got).all(), name
    judge(name, err_rows(got, r64, dim), err_rows(r32, r64, dim))


def check_scaled(name, got, r64, r32, scale):
    assert torch.isfinite(got).all(), name
    judge(name, err_scaled(got, r64, scale), err_scaled(r32, r64, scale))


def l2(summands, dim=0):
    return summands.double().pow(2).sum(dim).sqrt()


def seed_of(n):
    return K.DropCtx(DEV, seed=n).seed


def keep_rate_ok(keep, p):
    n = keep.numel()
    rate = keep.double().mean().item()
    print(f"keep rate {rate:.4f} of {n} (expected {1 - p:.2f}, 3 sigma = {3 * math.sqrt(p * (1 - p) / n):.4f})")
    return abs(rate - (1 - p)) <= 3 * math.sqrt(p * (1 - p) / n)


# ================================================================================================ BatchNorm
EPS_BN, MOM = 1e-5, 0.1
BN_SHAPES = [(2, 8), (63, 8), (64, 8), (100, 12), (150, 36), (150, 80), (5000, 512)]


@functools.lru_cache(maxsize=None)
def bn_ref(rows, C, offset, act, dtype, seed=0):
    i = N.bn_inputs(rows, C, offset, seed)
    return N.batch_norm_grads(i["x"], i["gamma"], i["beta"], EPS_BN, i["dy"], act=act, running_mean=i["running_mean"],
                              running_var=i["running_var"], momentum=MOM, dtype=dtype)


def bn_kernel(i, act, p=0.0, seed=None, off=0):
    """the three kernel-level calls of a training step on the inputs i -> dict of device tensors"""
    x, g, b, dy = dev(i["x"]), dev(i["gamma"]), dev(i["beta"]), dev(i["dy"])
    rm, rv, nbt = dev(i["running_mean"]).clone(), dev(i["running_var"]).clone(), torch.tensor(5, dtype=torch.int64, device=DEV)
    mean, rstd = K.bn_batch_stats(x, EPS_BN, MOM, rm, rv, nbt)
    y = K.bn_apply(x, mean, rstd, g, b, ACT[act], p, seed, off)
    dx, dg, db = K.bn_bwd(dy, x, mean, rstd, g, b, ACT[act], p, seed, off, True)
    return dict(mean=mean, rstd=rstd, y=y, dx=dx, dgamma=dg, dbeta=db, running_mean=rm, running_var=rv, nbt=nbt)


def bn_compare(tag, k, r64, r32, i, quantities):
    rows = i["x"].shape[0]
    for q in quantities:
        n = f"{tag} {q}"
        if q in ("y", "dx"):
            check_rows(n, k[q], r64[q], r32[q], 0)
        elif q in ("rstd", "running_var"):
            check_scaled(n, k[q], r64[q], r32[q], r64[q].abs())
        elif q == "mean":
            check_scaled(n, k[q], r64[q], r32[q], l2(i["x"]) / rows)
        elif q == "running_mean":
            check_scaled(n, k[q], r64[q], r32[q], (1 - MOM) * i["running_mean"].double().abs() + MOM * r64["mean"].abs())
        elif q == "dgamma":
            check_scaled(n, k[q], r64[q], r32[q], l2(r64["sg"]))
        elif q == "dbeta":
            check_scaled(n, k[q], r64[q], r32[q], l2(r64["sb"]))
        else:
            raise KeyError(q)


BN_ALL = ("mean", "rstd", "y", "dx", "dgamma", "dbeta", "running_mean", "running_var")


@pytest.mark.parametrize("act", N.ACTS)
@pytest.mark.parametrize("rows,C", BN_SHAPES)
def test_batchnorm_train_step_against_float64(rows, C, act):
    """no fold / fold x8 / fold x4 with a 48-wide view / scalar and wide apply kernels / 78 stripes in five groups (the last of 14)"""
    i = N.bn_inputs(rows, C)
    k = bn_kernel(i, act)
    bn_compare(f"bn [{rows}, {C}] {act}", k, bn_ref(rows, C, 0.0, act, D), bn_ref(rows, C, 0.0, act, F32), i, BN_ALL)
    assert int(k["nbt"]) == 5 + bn_ref(rows, C, 0.0, act, D)["num_batches_inc"]


@pytest.mark.parametrize("act", N.ACTS)
@pytest.mark.parametrize("rows,C", [(150, 36), (150, 80)])
def test_batchnorm_op_train_and_eval_against_float64(rows, C, act):
    """ops.batch_norm_act with autograd ([B, T, C] input): the training step, then eval mode on the running statistics it left"""
    i = N.bn_inputs(rows, C, offset=3.0, seed=1)
    r64, r32 = bn_ref(rows, C, 3.0, act, D, 1), bn_ref(rows, C, 3.0, act, F32, 1)
    x, g, b = [dev(i[q]).clone().requires_grad_() for q in ("x", "gamma", "beta")]
    rm, rv, nbt = dev(i["running_mean"]).clone(), dev(i["running_var"]).clone(), torch.tensor(0, dtype=torch.int64, device=DEV)
    y = ops.batch_norm_act(x.view(3, rows // 3, C), g, b, rm, rv, nbt, True, act=ACT[act], eps=EPS_BN, momentum=MOM)
    y.backward(dev(i["dy"]).view(3, rows // 3, C))
    k = dict(y=y.view(rows, C), dx=x.grad, dgamma=g.grad, dbeta=b.grad, running_mean=rm, running_var=rv)
    bn_compare(f"bn op [{rows}, {C}] {act}", k, r64, r32, i, ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var"))
    assert int(nbt) == 1
    # eval: both restatements start from the float32 running statistics the kernel left
    rm_c, rv_c = rm.cpu(), rv.cpu()
    e64 = N.batch_norm_grads(i["x"], i["gamma"], i["beta"], EPS_BN, i["dy"], act=act, training=False, running_mean=rm_c, running_var=rv_c)
    e32 = N.batch_norm_grads(i["x"], i["gamma"], i["beta"], EPS_BN, i["dy"], act=act, training=False, running_mean=rm_c, running_var=rv_c,
                             dtype=F32)
    x2, g2, b2 = [dev(i[q]).clone().requires_grad_() for q in ("x", "gamma", "beta")]
    ye = ops.batch_norm_act(x2.view(3, rows // 3, C), g2, b2, rm, rv, nbt, False, act=ACT[act], eps=EPS_BN, momentum=MOM)
    ye.backward(dev(i["dy"]).view(3, rows // 3, C))
    assert torch.equal(rm.cpu(), rm_c) and torch.equal(rv.cpu(), rv_c) and int(nbt) == 1, "eval mode must not touch the running statistics"
    bn_compare(f"bn op eval [{rows}, {C}] {act}", dict(y=ye.view(rows, C), dx=x2.grad, dgamma=g2.grad, dbeta=b2.grad), e64, e32, i,
               ("y", "dx", "dgamma", "dbeta"))


@pytest.mark.parametrize("offset", [0.0, 3.0, 30.0, 300.0])
@pytest.mark.parametrize("rows,C", [(150, 80), (4096, 32)])
def test_batchnorm_offset_sweep(rows, C, offset):
    """x = randn + offset * sign_c: channel means of up to 300 standard deviations.  The statistics must not lose digits to
    E[x^2] - mean^2 (stock float32 keeps rstd to 3e-8 on these inputs: tests/test_norm_restate_cpu.py)."""
    i = N.bn_inputs(rows, C, offset)
    k = bn_kernel(i, "none")
    bn_compare(f"bn offset {offset:g} [{rows}, {C}]", k, bn_ref(rows, C, offset, "none", D), bn_ref(rows, C, offset, "none", F32), i,
               ("mean", "rstd", "y", "dx"))


@pytest.mark.parametrize("rows,C", [(100, 12), (150, 36), (150, 80)])
def test_batchnorm_backward_accumulates_into_existing_gradients(rows, C):
    i = N.bn_inputs(rows, C, seed=2)
    x, g, b, dy = dev(i["x"]), dev(i["gamma"]), dev(i["beta"]), dev(i["dy"])
    mean, rstd = K.bn_batch_stats(x, EPS_BN, MOM, None, None, None)
    dx, dg, db = K.bn_bwd(dy, x, mean, rstd, g, b, K.ACT_TANH, 0.0, None, 0, True)
    pre_g, pre_b = dev(i["running_mean"]) * 3, dev(i["running_var"]) - 4
    buf_g, buf_b = pre_g.clone(), pre_b.clone()
    dx2, none_g, none_b = K.bn_bwd(dy, x, mean, rstd, g, b, K.ACT_TANH, 0.0, None, 0, True, acc_into=(buf_g, buf_b))
    assert none_g is None and none_b is None
    assert torch.equal(dx2, dx), "dx differs between the accumulating and the plain call"
    assert torch.equal(buf_g, pre_g + dg) and torch.equal(buf_b, pre_b + db)
    assert dg.abs().min() > 0 and db.abs().min() > 0


@pytest.mark.parametrize("rows,C", [(100, 12), (150, 36), (150, 80)])
def test_batchnorm_dropout_forward_and_backward_share_the_mask(rows, C):
    """p = 0.3, act = none, beta = 8 so that no pre-dropout output is 0: the keep-mask read from y, fed to the float64 restatement,
    must explain y and every gradient (folded view / scalar / wide kernels: each forms the element index its own way)"""
    p = 0.3
    i = dict(N.bn_inputs(rows, C, seed=3))
    i["beta"] = i["beta"] * 0 + 8.0
    i["gamma"] = i["gamma"].abs().clamp_min(0.5)
    k = bn_kernel(i, "none", p, seed_of(1234), off=3)
    keep = (k["y"] != 0).cpu()
    assert keep_rate_ok(keep, p)
    kw = dict(act="none", keep=keep, p=p, running_mean=i["running_mean"], running_var=i["running_var"], momentum=MOM)
    r64 = N.batch_norm_grads(i["x"], i["gamma"], i["beta"], EPS_BN, i["dy"], **kw)
    r32 = N.batch_norm_grads(i["x"], i["gamma"], i["beta"], EPS_BN, i["dy"], dtype=F32, **kw)
    z = N.batch_norm(i["x"], i["gamma"], i["beta"], EPS_BN)["y"]
    assert z.abs().min() > 1e-2, "the test needs non-zero pre-dropout outputs"
    bn_compare(f"bn dropout [{rows}, {C}]", k, r64, r32, i, ("y", "dx", "dgamma", "dbeta"))
    k2 = bn_kernel(i, "none", p, seed_of(1234), off=4)
    assert not torch.equal(k2["y"] != 0, k["y"] != 0), "another offset must draw another mask"


# ================================================================================================ LayerNorm
LN_SHAPES = ([(r, c) for c in (4, 252, 256) for r in (1, 5, 256, 257)] + [(r, c) for c in (260, 512) for r in (128, 131)]
             + [(r, c) for c in (516, 1024) for r in (64, 67)] + [(4100, 256)])


@functools.lru_cache(maxsize=None)
def ln_ref(rows, C, eps, dtype, with_dres, row_mean=0.0):
    i = N.ln_inputs(rows, C, row_mean=row_mean)
    return N.layer_norm_grads(i["x"], i["gamma"], i["beta"], eps, i["dy"], rowscale=i["rowscale"], dres=i["dres"] if with_dres else None,
                              dtype=dtype)


def ln_compare(tag, k, r64, r32, quantities=("mean", "rstd", "y", "dx", "dgamma", "dbeta"), x=None):
    for q in quantities:
        n = f"{tag} {q}"
        if q in ("y", "dx"):
            check_rows(n, k[q], r64[q], r32[q], -1)
        elif q == "rstd":
            check_scaled(n, k[q], r64[q], r32[q], r64[q].abs())
        elif q == "mean":
            check_scaled(n, k[q], r64[q], r32[q], l2(x, -1) / x.shape[-1])
        elif q == "dgamma":
            check_scaled(n, k[q], r64[q], r32[q], l2(r64["sg"]))
        elif q == "dbeta":
            check_scaled(n, k[q], r64[q], r32[q], l2(r64["sb"]))


def ln_kernel(i, eps, with_dres, p=0.0, seed=None, off=0, rowscale=True):
    x, g, b, dy = dev(i["x"]), dev(i["gamma"]), dev(i["beta"]), dev(i["dy"])
    rs = dev(i["rowscale"]) if rowscale else None
    y, mean, rstd = K.layernorm_fwd(x, g, b, eps, p, seed, off, rs)
    dx, dg, db = K.layernorm_bwd(dy, x, g, mean, rstd, p, seed, off, rs, dres=dev(i["dres"]) if with_dres else None)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dg, dbeta=db)


def ln_zero_rows(tag, k, i, with_dres):
    dead = i["rowscale"] == 0
    assert (k["y"].cpu()[dead] == 0).all(), f"{tag}: rows with rowscale 0 must be exactly 0"
    want = i["dres"][dead] if with_dres else torch.zeros_like(i["dres"][dead])
    assert torch.equal(k["dx"].cpu()[dead], want), f"{tag}: dx of a row with rowscale 0 must be exactly dres (or 0)"


@pytest.mark.parametrize("eps", [1e-12, 1e-5])
@pytest.mark.parametrize("rows,C", LN_SHAPES)
def test_layernorm_fwd_bwd_against_float64(rows, C, eps):
    """every template instantiation of the backward (C <= 256 / 512 / 1024) at its narrowest and widest C with a partial last lane
    group, at 1, exactly 16 and 17 workgroups (two reduction groups, 16 + 1, tail rows clamped and masked) and under the grid cap"""
    i = N.ln_inputs(rows, C)
    for with_dres in (False, True):
        tag = f"ln [{rows}, {C}] eps {eps:g}{' +dres' if with_dres else ''}"
        k = ln_kernel(i, eps, with_dres)
        ln_compare(tag, k, ln_ref(rows, C, eps, D, with_dres), ln_ref(rows, C, eps, F32, with_dres), x=i["x"],
                   quantities=("mean", "rstd", "y", "dx", "dgamma", "dbeta") if not with_dres else ("dx", "dgamma", "dbeta"))
        ln_zero_rows(tag, k, i, with_dres)


@pytest.mark.parametrize("rows,C", [(257, 256), (67, 1024)])
def test_layernorm_rows_with_a_large_mean(rows, C):
    """rows of mean +-1000 and a spread of about 1: the forward takes the variance around the mean (two passes over registers)"""
    i = N.ln_inputs(rows, C, row_mean=1000.0)
    k = ln_kernel(i, 1e-5, True)
    ln_compare(f"ln mean 1000 [{rows}, {C}]", k, ln_ref(rows, C, 1e-5, D, True, 1000.0), ln_ref(rows, C, 1e-5, F32, True, 1000.0), x=i["x"])


def test_layernorm_backward_without_a_workspace_is_one_workgroup_and_as_accurate():
    rows, C, eps = 257, 256, 1e-5
    i = N.ln_inputs(rows, C)
    x, g, b, dy, rs, dres = [dev(i[q]) for q in ("x", "gamma", "beta", "dy", "rowscale", "dres")]
    y, mean, rstd = K.layernorm_fwd(x, g, b, eps, 0.0, None, 0, rs)
    dx, dg, db = torch.empty_like(x), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    p = K._p
    _lib.check(_lib.load().ctts_layernorm_bwd(p(dy), p(x), p(g), p(mean), p(rstd), p(dx), p(dg), p(db), rows, C, 0.0, None, 0, p(rs), 0,
                                              p(dres), None, None, K._stream()), "ctts_layernorm_bwd")
    ln_compare("ln no workspace [257, 256]", dict(dx=dx, dgamma=dg, dbeta=db), ln_ref(rows, C, eps, D, True), ln_ref(rows, C, eps, F32, True),
               quantities=("dx", "dgamma", "dbeta"))
    dx_ws = K.layernorm_bwd(dy, x, g, mean, rstd, rowscale=rs, dres=dres)[0]
    assert torch.equal(dx, dx_ws), "dx does not depend on how the parameter sums are reduced"


@pytest.mark.parametrize("rows,C", [(257, 256), (131, 516)])
def test_layernorm_ops_against_float64(rows, C):
    """ops.layer_norm (rowscale) and ops.layer_norm_res (the residual gradient arrives in the same backward) through autograd"""
    eps = 1e-5
    i = N.ln_inputs(rows, C)
    x, g, b = [dev(i[q]).clone().requires_grad_() for q in ("x", "gamma", "beta")]
    y = ops.layer_norm(x, g, b, eps, rowscale=dev(i["rowscale"]))
    y.backward(dev(i["dy"]))
    ln_compare(f"ops.layer_norm [{rows}, {C}]", dict(y=y, dx=x.grad, dgamma=g.grad, dbeta=b.grad), ln_ref(rows, C, eps, D, False),
               ln_ref(rows, C, eps, F32, False), quantities=("y", "dx", "dgamma", "dbeta"))
    r64, r32 = [N.layer_norm_grads(i["x"], i["gamma"], i["beta"], eps, i["dy"], dres=i["dres"], dtype=t) for t in (D, F32)]
    x, g, b = [dev(i[q]).clone().requires_grad_() for q in ("x", "gamma", "beta")]
    y, xres = ops.layer_norm_res(x, g, b, eps)
    assert torch.equal(xres, x)
    ((y * dev(i["dy"])).sum() + (xres * dev(i["dres"])).sum()).backward()
    ln_compare(f"ops.layer_norm_res [{rows}, {C}]", dict(y=y, dx=x.grad, dgamma=g.grad, dbeta=b.grad), r64, r32,
               quantities=("y", "dx", "dgamma", "dbeta"))


@pytest.mark.parametrize("rows,C", [(257, 256), (131, 516), (67, 1024)])
def test_layernorm_dropout_forward_and_backward_share_the_mask(rows, C):
    p, eps = 0.5, 1e-5
    i = dict(N.ln_inputs(rows, C, seed=4))
    i["beta"] = i["beta"] * 0 + 3.0                    # beta = 3, gamma = 1: y has no true zeros, the mask can be read from it
    i["gamma"] = i["gamma"] * 0 + 1.0
    k = ln_kernel(i, eps, False, p, seed_of(4321), off=7, rowscale=False)
    keep = (k["y"] != 0).cpu()
    assert keep_rate_ok(keep, p)
    assert N.layer_norm(i["x"], i["gamma"], i["beta"], eps)["y"].abs().min() > 1e-4, "the test needs non-zero pre-dropout outputs"
    r64, r32 = [N.layer_norm_grads(i["x"], i["gamma"], i["beta"], eps, i["dy"], keep=keep, p=p, dtype=t) for t in (D, F32)]
    ln_compare(f"ln dropout [{rows}, {C}]", k, r64, r32, quantities=("y", "dx", "dgamma", "dbeta"))


# ================================================================================================ square masked softmax
SENTINEL = -12345.6787109375


def sq_lens(T):
    return [[1, 1]] if T == 1 else [[T // 2 + 1, T], [T, 1]]


@functools.lru_cache(maxsize=None)
def sq_ref(T, lens, dtype):
    S, dP = N.score_inputs((2, 2, T, T), seed=9)
    return N.softmax_grads(lambda s: N.softmax_square(s, lens, dtype), S, dP, dtype)


def region(T, lens):
    """bool [2, 2, T, T]: q < L and k < L"""
    ar = torch.arange(T)
    L = torch.tensor(lens)[:, None, None, None]
    return ((ar[None, None, :, None] < L) & (ar[None, None, None, :] < L)).expand(2, 2, T, T)


@pytest.mark.parametrize("T,lens", [(T, tuple(l)) for T in (1, 63, 64, 65, 1024, 1025, 1100) for l in sq_lens(T)])
def test_square_softmax_against_float64_and_leaves_the_padding_alone(T, lens):
    """L <= 1024 keeps the row in registers, longer rows stream it three times; for T > 1024 a launch holds rows of both kinds"""
    S, dP = N.score_inputs((2, 2, T, T), seed=9)
    valid = region(T, lens)
    buf = torch.where(valid, S, torch.tensor(SENTINEL)).to(DEV)
    before = buf.clone()
    K.softmax_fwd(buf, torch.tensor(lens, dtype=torch.int32, device=DEV), 2, 2, T)
    vd = valid.to(DEV)
    assert torch.equal(buf[~vd].view(torch.int32), before[~vd].view(torch.int32)), "forward wrote outside q < L, k < L"
    P = torch.where(vd, buf, torch.zeros((), device=DEV))
    (p64, d64), (p32, d32) = sq_ref(T, lens, D), sq_ref(T, lens, F32)
    for b, L in enumerate(lens):
        check_rows(f"softmax T {T} L {L} P", P[b, :, :L, :L], p64[b, :, :L, :L], p32[b, :, :L, :L], -1)
        dev_sum = (c64(P[b, :, :L, :L]).sum(-1) - 1).abs().max().item()
        print(f"softmax T {T} L {L}: max |row sum - 1| {dev_sum:.2e}  bound {FLOOR * math.sqrt(L):.2e}")
        assert dev_sum <= FLOOR * math.sqrt(L)
    g = torch.where(valid, dP, torch.tensor(SENTINEL)).to(DEV)
    g_before = g.clone()
    K.softmax_bwd(buf, g, torch.tensor(lens, dtype=torch.int32, device=DEV), 2, 2, T)
    assert torch.equal(g[~vd].view(torch.int32), g_before[~vd].view(torch.int32)), "backward wrote outside q < L, k < L"
    # the restatements differentiate their own P; the kernel was handed its own float32 P, as in the product
    for b, L in enumerate(lens):
        check_rows(f"softmax T {T} L {L} dS", g[b, :, :L, :L], d64[b, :, :L, :L], d32[b, :, :L, :L], -1)


# ================================================================================================ rectangular softmax
@pytest.mark.parametrize("with_qlens", [True, False], ids=["qlens", "no_qlens"])
@pytest.mark.parametrize("Tq,Tk", [(1, 1), (5, 32), (70, 65), (33, 300)])
def test_rect_softmax_against_float64_with_exact_zeros(Tq, Tk, with_qlens):
    klens = [0, 1, Tk, Tk, (Tk + 1) // 2]
    qlens = [Tq, Tq, Tq, 0, (Tq + 1) // 2] if with_qlens else None
    nb = len(klens)
    S, dP = N.score_inputs((nb, Tq, Tk), seed=10)
    kl = torch.tensor(klens, dtype=torch.int32, device=DEV)
    ql = torch.tensor(qlens, dtype=torch.int32, device=DEV) if with_qlens else None
    P = K.softmax_rect_fwd(dev(S).clone(), kl, ql)
    dS = K.softmax_rect_bwd(P, dev(dP).clone(), kl, ql)
    (p64, d64), (p32, d32) = [N.softmax_grads(lambda s: N.softmax_rect(s, klens, qlens, t), S, dP, t) for t in (D, F32)]
    zero = (p64 == 0)
    live_rows = 0
    for b in range(nb):
        L, Lq = klens[b], (qlens[b] if with_qlens else Tq)
        assert zero[b, Lq:].all() and zero[b, :, L:].all() and (L == 0 or not zero[b, :Lq, :L].any())
        live_rows += Lq if L > 0 else 0
    assert (P.cpu()[zero] == 0).all() and (dS.cpu()[zero] == 0).all(), "masked keys and dead rows must be exactly 0 in P and dS"
    assert live_rows > 0
    check_rows(f"rect softmax [{Tq}, {Tk}] P", P, p64, p32, -1)
    check_rows(f"rect softmax [{Tq}, {Tk}] dS", dS, d64, d32, -1)


# ================================================================================================ relative-position kernels
REL_T = (1, 2, 63, 64, 65, 130)


def rel_inputs(T):
    S, dP = N.score_inputs((3, T, T), seed=11)
    PS, _ = N.score_inputs((3, T, T), seed=12, spread=1.5)
    return S, PS, dP


def rel_ref(T, scale, dtype, keep=None, p=0.0):
    """-> (P, Pd, dS = gradient of <Pd, dP> with respect to S)"""
    S, PS, dP = rel_inputs(T)
    Sl = S.to(dtype).requires_grad_()
    P, Pd = N.relpos_softmax(Sl, PS, scale, keep, p, dtype)
    Pd.backward(dP.to(dtype))
    return P.detach(), Pd.detach(), Sl.grad


@pytest.mark.parametrize("scale", [0.25, 1.0])
@pytest.mark.parametrize("T", REL_T)
def test_relpos_softmax_against_float64(T, scale):
    S, PS, dP = rel_inputs(T)
    buf = dev(S).clone()
    Pd = K.relpos_softmax_fwd(buf, dev(PS), T, scale)
    assert torch.equal(Pd, buf), "without dropout the dropped copy is P itself"
    (p64, _, d64), (p32, _, d32) = rel_ref(T, scale, D), rel_ref(T, scale, F32)
    check_rows(f"relpos T {T} scale {scale} P", buf, p64, p32, -1)
    dS = K.relpos_softmax_bwd(buf, dev(dP).clone(), T, scale)
    check_rows(f"relpos T {T} scale {scale} dS", dS, d64, d32, -1)


@pytest.mark.parametrize("T", REL_T)
def test_relshift_backward_is_the_exact_adjoint_of_the_reference_shift(T):
    _, _, dS = rel_inputs(T)
    got = K.relshift_bwd(dev(dS), T).cpu()
    want = N.rel_shift_adjoint(dS)
    assert want.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "relshift_bwd is a pure gather: bit-equal to the float32 adjoint"


@pytest.mark.parametrize("T", [2, 65, 130])
def test_relpos_dropout_forward_and_backward_share_the_mask(T):
    p, scale = 0.2, 0.25
    S, PS, dP = rel_inputs(T)
    seed = seed_of(99)
    buf = dev(S).clone()
    Pd = K.relpos_softmax_fwd(buf, dev(PS), T, scale, p, seed, 5)
    assert (buf > 0).all(), "the test needs P > 0 to read the mask from Pd"
    keep = Pd != 0
    if T > 2:
        assert keep_rate_ok(keep, p)
    inv_keep = (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))).item()          # float32 arithmetic, as the kernel
    want = buf * keep * inv_keep
    assert torch.allclose(Pd, want, rtol=2.0 ** -22, atol=0.0), "Pd != P * mask / (1 - p)"
    (_, pd64, d64), (_, pd32, d32) = rel_ref(T, scale, D, keep.cpu(), p), rel_ref(T, scale, F32, keep.cpu(), p)
    check_rows(f"relpos dropout T {T} Pd", Pd, pd64, pd32, -1)
    dS = K.relpos_softmax_bwd(buf, dev(dP).clone(), T, scale, p, seed, 5)
    check_rows(f"relpos dropout T {T} dS", dS, d64, d32, -1)
