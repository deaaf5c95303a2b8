"""Plain-torch restatement of the normalisation and softmax kernels of csrc/norm.hip (LayerNorm, BatchNorm1d, masked square softmax),
csrc/prosody.hip (rectangular softmax) and csrc/conformer.hip (relative-position softmax and shift) - the oracle of
tests/test_norm_kernels_gpu.py (run in float64; the same code in float32 is the stock-torch yardstick the tests print).

Written from the kernel headers and include/ctts.h: elementary tensor arithmetic with autograd on the CPU only, dropout as an explicit
keep-mask with the 1 / (1 - p) scale; no product code and no oracle code is called.  tests/test_norm_restate_cpu.py pins every function
against the stock op (F.layer_norm, F.batch_norm, torch.softmax with masked_fill, the padded.view shift of the reference)."""
import torch
import torch.nn.functional as F

ACTS = ("none", "tanh", "swish")


def _drop(y, keep, p, dtype):
    return y if keep is None else y * (keep.to(dtype) / (1.0 - p))


def _act(z, act):
    if act == "none":
        return z
    if act == "tanh":
        return torch.tanh(z)
    if act == "swish":
        return z * torch.sigmoid(z)
    raise ValueError(act)


# ------------------------------------------------------------------------------------------------ LayerNorm
def layer_norm(x, gamma, beta, eps, rowscale=None, keep=None, p=0.0, dtype=torch.float64):
    """x [rows, C] -> dict(y = rowscale * drop(LN(x)), mean [rows], rstd [rows], xh = (x - mean) * rstd, z = xh * gamma + beta).
    Biased variance, taken around the mean.  x, gamma, beta keep their autograd history when they already have `dtype`; z retains its
    gradient (the summands of dgamma / dbeta are z.grad * xh / z.grad)."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    z = xh * gamma + beta
    if z.requires_grad:
        z.retain_grad()
    y = _drop(z, keep, p, dtype)
    if rowscale is not None:
        y = y * rowscale.to(dtype)[:, None]
    return dict(y=y, mean=mean[:, 0], rstd=rstd[:, 0], xh=xh, z=z)


def layer_norm_grads(x, gamma, beta, eps, dy, rowscale=None, keep=None, p=0.0, dres=None, dtype=torch.float64):
    """forward + autograd backward under the upstream gradient dy; dres (the gradient of a residual branch that carries x itself) is
    added to dx.  -> dict of detached tensors: y, mean, rstd, dx, dgamma, dbeta and the per-element summands sg (of dgamma), sb (of dbeta)"""
    xl, gl, bl = [t.detach().to(dtype).clone().requires_grad_() for t in (x, gamma, beta)]
    r = layer_norm(xl, gl, bl, eps, rowscale, keep, p, dtype)
    r["y"].backward(dy.to(dtype))
    dx = xl.grad if dres is None else xl.grad + dres.to(dtype)
    return dict(y=r["y"].detach(), mean=r["mean"].detach(), rstd=r["rstd"].detach(), dx=dx, dgamma=gl.grad, dbeta=bl.grad,
                sg=(r["z"].grad * r["xh"]).detach(), sb=r["z"].grad.detach())


# ------------------------------------------------------------------------------------------------ BatchNorm1d, channel-last
def batch_stats(x, eps, dtype=torch.float64):
    """x [rows, C] -> (mean [C], biased variance [C], rstd [C]) over all rows"""
    x = x.to(dtype)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def running_update(mean, var_biased, rows, running_mean, running_var, momentum, dtype=torch.float64):
    """nn.BatchNorm1d's update: (1 - m) * running + m * (batch mean | UNBIASED batch variance); -> (running_mean, running_var, 1 = the
    num_batches_tracked increment).  rows == 1 keeps the biased variance (divisor max(rows - 1, 1), as the kernel)."""
    unbiased = var_biased.to(dtype) * (rows / max(rows - 1, 1))
    return ((1.0 - momentum) * running_mean.to(dtype) + momentum * mean.to(dtype),
            (1.0 - momentum) * running_var.to(dtype) + momentum * unbiased, 1)


def batch_norm(x, gamma, beta, eps, act="none", keep=None, p=0.0, training=True, running_mean=None, running_var=None, momentum=0.1,
               dtype=torch.float64):
    """x [rows, C] -> dict(y = drop(act(BN(x))), mean, rstd, xh, z = xh * gamma + beta (retains its gradient), and in training mode
    running_mean / running_var / num_batches_inc = the updated running statistics).  training: batch statistics (biased variance);
    else the running statistics."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    out = {}
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        if running_mean is not None:
            out["running_mean"], out["running_var"], out["num_batches_inc"] = running_update(
                mean.detach(), var.detach(), x.shape[0], running_mean, running_var, momentum, dtype)
    else:
        mean, var = running_mean.to(dtype), running_var.to(dtype)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    z = xh * gamma + beta
    if z.requires_grad:
        z.retain_grad()
    out.update(y=_drop(_act(z, act), keep, p, dtype), mean=mean, rstd=rstd, xh=xh, z=z)
    return out


def batch_norm_grads(x, gamma, beta, eps, dy, act="none", keep=None, p=0.0, training=True, running_mean=None, running_var=None,
                     momentum=0.1, dtype=torch.float64):
    """forward + autograd backward; -> dict of detached tensors: y, mean, rstd, dx, dgamma, dbeta, sg / sb (summands of dgamma / dbeta)
    and the running-statistics update in training mode"""
    xl, gl, bl = [t.detach().to(dtype).clone().requires_grad_() for t in (x, gamma, beta)]
    r = batch_norm(xl, gl, bl, eps, act, keep, p, training, running_mean, running_var, momentum, dtype)
    r["y"].backward(dy.to(dtype))
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in r.items() if k not in ("xh", "z")}
    out.update(dx=xl.grad, dgamma=gl.grad, dbeta=bl.grad, sg=(r["z"].grad * r["xh"]).detach(), sb=r["z"].grad.detach())
    return out


# ------------------------------------------------------------------------------------------------ softmax over keys
def softmax_square(S, lens, dtype=torch.float64):
    """S [nb0, nb1, T, T], lens [nb0] -> P: softmax over keys k < L of the rows q < L (L = min(lens[b], T)), 0 everywhere else (the
    kernel leaves those elements as they were: the caller compares the valid region only)."""
    S = S.to(dtype)
    nb0, _, T, _ = S.shape
    out = []
    for b in range(nb0):
        L = max(min(int(lens[b]), T), 0)
        s = S[b, :, :L, :L]
        e = torch.exp(s - s.amax(-1, keepdim=True).detach()) if L else s
        out.append(F.pad(e / e.sum(-1, keepdim=True), (0, T - L, 0, T - L)))
    return torch.stack(out)


def softmax_rect(S, klens=None, qlens=None, dtype=torch.float64):
    """S [nb, Tq, Tk] -> P: softmax over the keys k < klens[b]; keys >= klens[b] come out 0; query rows >= qlens[b] and all rows of a
    batch entry with klens[b] == 0 are all zero.  None = full length."""
    S = S.to(dtype)
    nb, Tq, Tk = S.shape
    out = []
    for b in range(nb):
        L = Tk if klens is None else min(int(klens[b]), Tk)
        Lq = Tq if qlens is None else min(int(qlens[b]), Tq)
        L, Lq = max(L, 0), max(Lq, 0)
        if L == 0 or Lq == 0:
            out.append(S[b] * 0.0)
            continue
        s = S[b, :Lq, :L]
        e = torch.exp(s - s.amax(-1, keepdim=True).detach())
        out.append(F.pad(e / e.sum(-1, keepdim=True), (0, Tk - L, 0, Tq - Lq)))
    return torch.stack(out)


def softmax_grads(fn, S, dP, dtype=torch.float64):
    """-> (P, dS) of P = fn(S leaf in dtype) under the upstream gradient dP"""
    Sl = S.detach().to(dtype).clone().requires_grad_()
    P = fn(Sl)
    P.backward(dP.to(dtype))
    return P.detach(), Sl.grad


# ------------------------------------------------------------------------------------------------ relative-position scores
def rel_shift(PS):
    """PS [nb, T, T] -> shifted [nb, T, T], the reference's way: a zero column in front, the [T, T + 1] slab viewed as [T + 1, T], its
    first row dropped.  shifted.flat[i * T + j] = padded.flat[i * T + j + T]."""
    nb, T, _ = PS.shape
    padded = torch.cat([PS.new_zeros(nb, T, 1), PS], dim=-1)
    return padded.reshape(nb, T + 1, T)[:, 1:].reshape(nb, T, T)


def rel_shift_adjoint(dS):
    """the adjoint of rel_shift by autograd: dPS with <rel_shift(PS), dS> = <PS, dPS>.  A pure gather: exact in every dtype."""
    PS = torch.zeros_like(dS).requires_grad_()
    rel_shift(PS).backward(dS)
    return PS.grad


def relpos_softmax(S, PS, scale, keep=None, p=0.0, dtype=torch.float64):
    """-> (P = softmax((S + rel_shift(PS)) * scale) over the last dim, Pd = drop(P))"""
    v = (S.to(dtype) + rel_shift(PS.to(dtype))) * scale
    e = torch.exp(v - v.amax(-1, keepdim=True).detach())
    P = e / e.sum(-1, keepdim=True)
    return P, _drop(P, keep, p, dtype)


# ------------------------------------------------------------------------------------------------ seeded inputs of the GPU tests
def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1, 7919, 104729, 1299709))) % (2 ** 31))


def bn_inputs(rows, C, offset=0.0, seed=0):
    """float32 CPU tensors: x = randn + offset * sign_c (sign_c = +1 / -1 on even / odd channels), gamma in +-[0.5, 1.5] with channel 0
    scaled to 1e-3 (a small-magnitude channel), beta, the upstream gradient dy and non-trivial running statistics"""
    g = _gen(rows, C, int(offset), seed)
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    x = torch.randn(rows, C, generator=g) + float(offset) * sign
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    gamma[0] *= 1e-3
    return dict(x=x, gamma=gamma, beta=torch.randn(C, generator=g) * 0.5, dy=torch.randn(rows, C, generator=g),
                running_mean=torch.randn(C, generator=g), running_var=torch.rand(C, generator=g) + 0.5)


def ln_inputs(rows, C, seed=0, row_mean=0.0):
    """float32 CPU tensors: x with per-row spread in [0.5, 2] (+ row_mean with alternating sign), gamma, beta, dy, a rowscale with zeros
    (and values other than 1) and a residual gradient dres"""
    g = _gen(rows, C, int(row_mean), seed)
    x = torch.randn(rows, C, generator=g) * (torch.rand(rows, 1, generator=g) * 1.5 + 0.5)
    x = x + float(row_mean) * torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)[:, None]
    u = torch.rand(rows, generator=g)
    rowscale = torch.where(u < 0.3, 0.0, torch.where(u < 0.6, 1.0, u * 2))
    rowscale[0] = 1.5                                   # a single row stays live; the second row is always a zero row
    if rows > 1:
        rowscale[1] = 0.0
    return dict(x=x, gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.5, dy=torch.randn(rows, C, generator=g),
                rowscale=rowscale, dres=torch.randn(rows, C, generator=g))


def score_inputs(shape, seed=0, spread=3.0):
    """(scores, upstream gradient) float32 CPU tensors of `shape`; the scores have a per-row spread of up to `spread`"""
    g = _gen(*shape[-3:], seed)
    s = torch.randn(*shape, generator=g) * (torch.rand(*shape[:-1], 1, generator=g) * spread)
    return s, torch.randn(*shape, generator=g)
