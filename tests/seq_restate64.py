"""Plain-torch restatement of the sequence kernels of csrc/conformer.hip (GLU, depthwise Conv1d forward / data gradient / weight
gradient, relattn_split) and csrc/prosody.hip (the GRU recurrence and its BPTT, the 3x3 stride-(1,2) Conv2d patch matrix and its
adjoint) - the oracle of tests/test_seq_kernels_gpu.py (run in float64; the same code in float32 is the stock-torch yardstick the tests
print).

Written from the kernel headers and include/ctts.h: elementary tensor arithmetic on the CPU with the kernels' layouts; the gradients
are written out by hand (tests/test_seq_restate_cpu.py pins them against autograd through torch.nn.GRU, F.conv1d, F.glu, F.unfold and
F.conv2d).  No product code and no oracle code is called.  Every function returns what the kernels emit; where a result is a sum it
also returns the L2 norm of the summands (`*_norm`), the scale a rounding error of that sum is measured against."""
import torch
import torch.nn.functional as F


def _sq(t):
    return t * t


# ------------------------------------------------------------------------------------------------ GRU
def gru(gi, whh, bhh, rev_mask=0, dout=None, dtype=torch.float64):
    """The recurrent part of a one-layer GRU with h0 = 0, `ndir` independent sequences per utterance.
    gi [B,T,ndir,3H] = W_ih x + b_ih (r | z | n), whh [ndir,3H,H], bhh [ndir,3H]; bit d of rev_mask: sequence d runs t = T-1 .. 0.
    -> dict(out [B,T,ndir,H], gates [B,T,ndir,4H] = r | z | n | W_hn h + b_hn, hprev [B,T,ndir,H] = the state each step started from)
    and, under the upstream gradient dout [B,T,ndir,H], by hand-written BPTT: dgi, dgh [B,T,ndir,3H] (gradients of the input and of
    the hidden projection W_hh h + b_hh), dwhh [ndir,3H,H] = sum_{b,t} dgh (x) hprev, dbhh [ndir,3H] = sum_{b,t} dgh, and
    dwhh_norm / dbhh_norm, the L2 norms of those summands over (b, t)."""
    gi, whh, bhh = gi.to(dtype), whh.to(dtype), bhh.to(dtype)
    B, T, ndir, H3 = gi.shape
    H = H3 // 3
    out, hprev, gates = gi.new_zeros(B, T, ndir, H), gi.new_zeros(B, T, ndir, H), gi.new_zeros(B, T, ndir, 4 * H)
    for d in range(ndir):
        rev = (rev_mask >> d) & 1
        h = gi.new_zeros(B, H)
        for s in range(T):
            t = T - 1 - s if rev else s
            gh = h @ whh[d].t() + bhh[d]
            r = torch.sigmoid(gi[:, t, d, :H] + gh[:, :H])
            z = torch.sigmoid(gi[:, t, d, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gi[:, t, d, 2 * H:] + r * gh[:, 2 * H:])
            hprev[:, t, d] = h
            h = (1.0 - z) * n + z * h
            out[:, t, d] = h
            gates[:, t, d] = torch.cat([r, z, n, gh[:, 2 * H:]], -1)
    res = dict(out=out, gates=gates, hprev=hprev)
    if dout is None:
        return res
    dout = dout.to(dtype)
    dgi, dgh = torch.zeros_like(gi), torch.zeros_like(gi)
    for d in range(ndir):
        rev = (rev_mask >> d) & 1
        dh = gi.new_zeros(B, H)
        for s in range(T - 1, -1, -1):
            t = T - 1 - s if rev else s
            r, z, n, ghn = gates[:, t, d].split(H, -1)
            hp = hprev[:, t, d]
            g = dh + dout[:, t, d]
            dn = g * (1.0 - z)
            dz = g * (hp - n)
            dnp = dn * (1.0 - n * n)
            dzp = dz * z * (1.0 - z)
            drp = dnp * ghn * r * (1.0 - r)
            dgi[:, t, d] = torch.cat([drp, dzp, dnp], -1)
            dgh[:, t, d] = torch.cat([drp, dzp, dnp * r], -1)
            dh = g * z + dgh[:, t, d] @ whh[d]
    res.update(dgi=dgi, dgh=dgh,
               dwhh=torch.einsum("btdi,btdj->dij", dgh, hprev), dwhh_norm=torch.einsum("btdi,btdj->dij", _sq(dgh), _sq(hprev)).sqrt(),
               dbhh=dgh.sum((0, 1)), dbhh_norm=_sq(dgh).sum((0, 1)).sqrt())
    return res


# ------------------------------------------------------------------------------------------------ depthwise Conv1d, channel-last
def dwconv(x, w, dy=None, dtype=torch.float64):
    """'same' depthwise convolution without bias: x [B,T,C], w [C,K] (K odd) -> y[b,t,c] = sum_k w[c,k] x[b,t+k-pad,c], pad = (K-1)/2,
    x = 0 outside [0, T).  -> dict(y, y_norm = L2 norm over the K taps of the summands) and, under the upstream gradient dy [B,T,C]:
    dx[b,u,c] = sum_k w[c,k] dy[b,u-k+pad,c] with dx_norm over the taps; dw[c,k] = sum_{b,t} dy[b,t,c] x[b,t+k-pad,c] with dw_norm
    over (b, t)."""
    x, w = x.to(dtype), w.to(dtype)
    B, T, C = x.shape
    K = w.shape[1]
    pad = (K - 1) // 2
    xp = F.pad(x, (0, 0, pad, pad))
    y, y2 = torch.zeros_like(x), torch.zeros_like(x)
    for k in range(K):
        term = w[:, k] * xp[:, k:k + T]
        y += term
        y2 += _sq(term)
    res = dict(y=y, y_norm=y2.sqrt())
    if dy is None:
        return res
    dy = dy.to(dtype)
    dyp = F.pad(dy, (0, 0, pad, pad))
    dx, dx2 = torch.zeros_like(x), torch.zeros_like(x)
    dw, dw2 = torch.zeros_like(w), torch.zeros_like(w)
    for k in range(K):
        term = w[:, k] * dyp[:, 2 * pad - k:2 * pad - k + T]
        dx += term
        dx2 += _sq(term)
        term = dy * xp[:, k:k + T]
        dw[:, k] = term.sum((0, 1))
        dw2[:, k] = _sq(term).sum((0, 1))
    res.update(dx=dx, dx_norm=dx2.sqrt(), dw=dw, dw_norm=dw2.sqrt())
    return res


# ------------------------------------------------------------------------------------------------ GLU over the last dim
def glu(a, dout=None, dtype=torch.float64):
    """a [..., 2C] = x | g -> dict(out = x * sigmoid(g)) and, under dout, da = dout * s | dout * x * s * (1 - s)"""
    a = a.to(dtype)
    Cc = a.shape[-1] // 2
    x, g = a[..., :Cc], a[..., Cc:]
    s = torch.sigmoid(g)
    res = dict(out=x * s)
    if dout is not None:
        dout = dout.to(dtype)
        res["da"] = torch.cat([dout * s, dout * x * s * (1.0 - s)], -1)
    return res


# ------------------------------------------------------------------------------------------------ relattn_split
def relattn_split(qkv, u_bias, v_bias, dtype=torch.float64):
    """qkv [..., 3C] = q | k | v -> (qu = q + u_bias, qv = q + v_bias, kv = k | v)"""
    qkv, u_bias, v_bias = qkv.to(dtype), u_bias.to(dtype), v_bias.to(dtype)
    Cc = qkv.shape[-1] // 3
    q = qkv[..., :Cc]
    return q + u_bias, q + v_bias, qkv[..., Cc:].clone()


def relattn_split_bwd(dqu, dqv, dkv, dtype=torch.float64):
    """-> dqkv [..., 3C] = (dqu + dqv) | dkv"""
    return torch.cat([dqu.to(dtype) + dqv.to(dtype), dkv.to(dtype)], -1)


# ------------------------------------------------------------------------------------------------ Conv2d 3x3, stride (1,2), padding (1,1)
def _wo(W):
    return (W - 1) // 2 + 1


def im2col_3x3s2(x):
    """x [B,T,W,C] channel-last -> col [B*T*Wo, 9*C], Wo = (W-1)//2 + 1: col[(b,t,wo)][(kh,kw,c)] = x[b, t+kh-1, 2*wo-1+kw, c], 0
    outside the image.  A pure gather: exact in every dtype."""
    B, T, W, C = x.shape
    Wo = _wo(W)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    taps = [xp[:, kh:kh + T, kw:kw + 2 * Wo - 1:2] for kh in range(3) for kw in range(3)]
    return torch.stack(taps, 3).reshape(B * T * Wo, 9 * C)


def col2im_3x3s2(dcol, B, T, W, C, dtype=torch.float64):
    """the adjoint of im2col_3x3s2: dcol [B*T*Wo, 9*C] -> (dx [B,T,W,C], dx_norm = L2 norm of the at most 6 patch entries each
    input element collects)"""
    Wo = _wo(W)
    d = dcol.to(dtype).reshape(B, T, Wo, 9, C)
    acc, acc2 = d.new_zeros(B, T + 2, W + 2, C), d.new_zeros(B, T + 2, W + 2, C)
    for kh in range(3):
        for kw in range(3):
            tap = d[:, :, :, kh * 3 + kw]
            acc[:, kh:kh + T, kw:kw + 2 * Wo - 1:2] += tap
            acc2[:, kh:kh + T, kw:kw + 2 * Wo - 1:2] += _sq(tap)
    return acc[:, 1:T + 1, 1:W + 1].contiguous(), acc2[:, 1:T + 1, 1:W + 1].sqrt()


# ------------------------------------------------------------------------------------------------ seeded inputs of the GPU tests
def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1, 7919, 104729, 1299709, 15485863))) % (2 ** 31))


def gru_inputs(B, T, H, ndir, seed=0, gi_scale=1.0, spike=0.0):
    """float32 CPU tensors gi [B,T,ndir,3H], whh [ndir,3H,H] and bhh [ndir,3H] (uniform in +-1/sqrt(H), as nn.GRU initialises them) and
    the upstream gradient dout [B,T,ndir,H]; every utterance, direction and unit draws its own values.  gi = randn * gi_scale; spike > 0
    overwrites one element in 16 with +-spike."""
    g = _gen(B, T, H, ndir, seed)
    gi = torch.randn(B, T, ndir, 3 * H, generator=g) * gi_scale
    if spike:
        u = torch.rand(B, T, ndir, 3 * H, generator=g)
        gi = torch.where(u < 1 / 32, torch.tensor(float(spike)), torch.where(u < 1 / 16, torch.tensor(-float(spike)), gi))
    bound = H ** -0.5
    whh = (torch.rand(ndir, 3 * H, H, generator=g) * 2 - 1) * bound
    bhh = (torch.rand(ndir, 3 * H, generator=g) * 2 - 1) * bound
    return dict(gi=gi, whh=whh, bhh=bhh, dout=torch.randn(B, T, ndir, H, generator=g))


def dw_inputs(B, T, C, K, seed=0):
    """float32 CPU tensors x, dy [B,T,C], w [C,K] (taps of about 1/sqrt(K), every channel its own) and old [C,K], a non-zero gradient
    buffer for the accumulating weight gradient"""
    g = _gen(B, T, C, K, seed)
    return dict(x=torch.randn(B, T, C, generator=g), dy=torch.randn(B, T, C, generator=g),
                w=torch.randn(C, K, generator=g) * K ** -0.5, old=torch.randn(C, K, generator=g) * 3)


def glu_inputs(rows, C, seed=0, extremes=True):
    """float32 CPU tensors a [rows, 2C] = x | g and dout [rows, C]; with extremes the first eight gates are +-30 and +-100 (twice)"""
    g = _gen(rows, C, seed)
    a = torch.randn(rows, 2 * C, generator=g)
    a[:, C:] *= 3
    if extremes:
        vals = torch.tensor([30.0, -30.0, 100.0, -100.0, -100.0, 100.0, -30.0, 30.0])
        flat = a[:, C:].clone().reshape(-1)
        n = min(8, flat.numel())
        flat[:n] = vals[:n]
        a[:, C:] = flat.view(rows, C)
    return dict(a=a, dout=torch.randn(rows, C, generator=g))


def split_inputs(rows, C, seed=0):
    g = _gen(rows, C, seed)
    return dict(qkv=torch.randn(rows, 3 * C, generator=g), u=torch.randn(C, generator=g), v=torch.randn(C, generator=g),
                dqu=torch.randn(rows, C, generator=g), dqv=torch.randn(rows, C, generator=g), dkv=torch.randn(rows, 2 * C, generator=g))


def patch_inputs(B, T, W, C, seed=0):
    """float32 CPU tensors x [B,T,W,C] and dcol [B*T*Wo, 9*C]"""
    g = _gen(B, T, W, C, seed)
    return dict(x=torch.randn(B, T, W, C, generator=g), dcol=torch.randn(B * T * _wo(W), 9 * C, generator=g))
