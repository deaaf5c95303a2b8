"""float64 restatement of the two attention operators of csrc/attn.hip and of their unfused twins (ops._SelfAttention,
ops._RelPosAttention) in plain torch / numpy - no project kernel, no autograd: the oracle of tests/test_attention_gpu.py.

Every function returns its tensors together with their *magnitude versions*: the same expression with every factor replaced by its
absolute value and the probabilities P kept as they are (out_mag = P |v|, dv_mag = P^T |dO|, dS_mag = P (|dO| |v|^T + rowsum(|dO| (P |v|))),
...).  That is the size of the terms a sum is made of, i.e. what rounding errors are proportional to.  The plain maximum of the result
is no usable normaliser: dq and dk cancel to nearly zero when a softmax row saturates.

`dtype=torch.float32` runs the very same statements on stock float32: the yardstick of a kernel's error on a given input."""
from collections import namedtuple

import numpy as np
import torch

Fs2 = namedtuple("Fs2", "out lse dq dk dv mag")                      # mag: dict with the same names
Rel = namedtuple("Rel", "out lse dqu dqv dkv dpos mag")
FS2_PARTS = ("out", "lse", "dq", "dk", "dv")
REL_PARTS = ("out", "lse", "dqu", "dqv", "dk", "dv", "dpos")        # dkv = dk | dv are compared one by one


def _heads(x, H):
    """[B,T,H*dh] -> [B,H,T,dh]"""
    B, T, C = x.shape
    return x.reshape(B, T, H, C // H).transpose(1, 2)


def _merge(x):
    """[B,H,T,dh] -> [B,T,H*dh]"""
    B, H, T, dh = x.shape
    return x.transpose(1, 2).reshape(B, T, H * dh)


def _softmax_lse(s, valid):
    """s [B,H,T,T] scores, valid [B,1|H,T,T] bool -> (P, lse): P = exp(s - lse) on the valid elements and 0 elsewhere; a row without a
    valid element has P = 0 and lse = 0"""
    sm = s.masked_fill(~valid, float("-inf"))
    m = sm.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(valid, torch.exp(sm - m), torch.zeros_like(s))
    tot = e.sum(-1, keepdim=True)
    live = tot > 0
    lse = torch.where(live, m + torch.log(torch.where(live, tot, torch.ones_like(tot))), torch.zeros_like(tot))
    P = torch.where(valid & live, torch.exp(sm - lse), torch.zeros_like(s))
    return P, lse[..., 0]


def _lse_mag(P, s, s_mag, lse):
    """lse = sum_j P_j (s_j - ln P_j) exactly; its magnitude version sum_j P_j (s_mag_j + |ln P_j|), with -ln P_j = lse - s_j"""
    neg_log_p = torch.where(P > 0, (lse[..., None] - s).abs(), torch.zeros_like(s))
    return (P * (s_mag + neg_log_p)).sum(-1)


def fs2_attention(qkv, lens, H, dout, dtype=torch.float64):
    """ops._SelfAttention: qkv [B,T,3C] packed q | k | v, lens [B] or None, dout [B,T,C].  q is scaled by d_h^-0.5, keys >= len get
    -inf, query rows >= len are zero rows (lens are clamped to T; an utterance of length 0 is all zero rows).
    -> Fs2(out [B,T,C], lse [B,H,T] natural log (0 at rows >= len), dq, dk, dv [B,T,C], mag)"""
    B, T, C3 = qkv.shape
    C = C3 // 3
    dh = C // H
    scale = dh ** -0.5
    x = qkv.detach().cpu().to(dtype)
    q, k, v = (_heads(t, H) for t in x.split(C, dim=-1))
    dO = _heads(dout.detach().cpu().to(dtype), H)
    L = torch.full((B,), T, dtype=torch.int64) if lens is None else torch.as_tensor(lens).cpu().to(torch.int64).clamp(max=T)
    ok = torch.arange(T)[None, :] < L[:, None]                      # [B,T]
    valid = (ok[:, None, :, None] & ok[:, None, None, :]).expand(B, H, T, T)
    s = (q * scale) @ k.transpose(-1, -2)
    P, lse = _softmax_lse(s, valid)
    out = P @ v
    dv = P.transpose(-1, -2) @ dO
    dP = dO @ v.transpose(-1, -2)
    D = (dO * out).sum(-1, keepdim=True)
    dS = P * (dP - D)
    dq = scale * (dS @ k)
    dk = scale * (dS.transpose(-1, -2) @ q)
    qa, ka, va, da = q.abs(), k.abs(), v.abs(), dO.abs()
    out_mag = P @ va
    dS_mag = P * (da @ va.transpose(-1, -2) + (da * out_mag).sum(-1, keepdim=True))
    mag = {"out": _merge(out_mag), "lse": _lse_mag(P, s, (qa * scale) @ ka.transpose(-1, -2), lse),
           "dq": _merge(scale * (dS_mag @ ka)), "dk": _merge(scale * (dS_mag.transpose(-1, -2) @ qa)),
           "dv": _merge(P.transpose(-1, -2) @ da)}
    return Fs2(_merge(out), lse, _merge(dq), _merge(dk), _merge(dv), mag)


def rel_shift(ps):
    """the conformer's shift (pad with a zero column, view as [T+1, T], drop the first row) on [B,H,T,T]"""
    B, H, T, _ = ps.shape
    padded = torch.cat([ps.new_zeros(B, H, T, 1), ps], dim=-1).reshape(B, H, T + 1, T)
    return padded[:, :, 1:].reshape(B, H, T, T)


def rel_unshift(g):
    """adjoint of rel_shift: the gradient of the unshifted scores from the gradient of the shifted ones"""
    B, H, T, _ = g.shape
    padded = torch.cat([g.new_zeros(B, H, 1, T), g], dim=2).reshape(B, H, T, T + 1)
    return padded[..., 1:]


def rel_attention(qu, qv, kv, pos, H, scale, dout, keep=None, p_drop=0.0, dtype=torch.float64):
    """ops._RelPosAttention: qu = q + u, qv = q + v [B,T,C], kv [B,T,2C] (k | v), pos [T,C], dout [B,T,C], keep bool [B,H,T,T] or None.
    score = (qu k^T + shift(qv pos^T)) * scale, softmax over all keys, kept probabilities scaled by 1/(1-p), context = Pd v.
    -> Rel(out [B,T,C], lse [B,H,T] natural log, dqu, dqv [B,T,C], dkv [B,T,2C], dpos [T,C] summed over the batch, mag); mag has the
    keys of REL_PARTS (dk and dv apart)"""
    B, T, C = qu.shape
    c = lambda t: t.detach().cpu().to(dtype)                       # noqa: E731
    q1, q2, k, v = _heads(c(qu), H), _heads(c(qv), H), _heads(c(kv)[..., :C], H), _heads(c(kv)[..., C:], H)
    p = c(pos).reshape(T, H, C // H).permute(1, 0, 2)[None]          # [1,H,T,dh]
    dO = _heads(c(dout), H)
    ks = torch.ones(B, H, T, T, dtype=dtype) if keep is None else torch.as_tensor(keep).cpu().to(dtype) / (1.0 - p_drop)
    s = (q1 @ k.transpose(-1, -2) + rel_shift(q2 @ p.transpose(-1, -2))) * scale
    P, lse = _softmax_lse(s, torch.ones_like(s, dtype=torch.bool))
    Pd = P * ks
    out = Pd @ v
    dv = Pd.transpose(-1, -2) @ dO
    dP = (dO @ v.transpose(-1, -2)) * ks
    D = (dO * out).sum(-1, keepdim=True)
    dS = P * (dP - D) * scale
    dqu = dS @ k
    dk = dS.transpose(-1, -2) @ q1
    dPS = rel_unshift(dS)
    dqv = dPS @ p
    dpos = (dPS.transpose(-1, -2) @ q2).sum(0)                       # [H,T,dh]
    a1, a2, ka, va, pa, da = q1.abs(), q2.abs(), k.abs(), v.abs(), p.abs(), dO.abs()
    out_mag = Pd @ va
    dS_mag = P * ((da @ va.transpose(-1, -2)) * ks + (da * out_mag).sum(-1, keepdim=True)) * scale
    dPS_mag = rel_unshift(dS_mag)
    s_mag = (a1 @ ka.transpose(-1, -2) + rel_shift(a2 @ pa.transpose(-1, -2))) * scale
    mag = {"out": _merge(out_mag), "lse": _lse_mag(P, s, s_mag, lse), "dqu": _merge(dS_mag @ ka), "dqv": _merge(dPS_mag @ pa),
           "dk": _merge(dS_mag.transpose(-1, -2) @ a1), "dv": _merge(Pd.transpose(-1, -2) @ da),
           "dpos": (dPS_mag.transpose(-1, -2) @ a2).sum(0).transpose(0, 1).reshape(T, C)}
    return Rel(_merge(out), lse, _merge(dqu), _merge(dqv), torch.cat([_merge(dk), _merge(dv)], -1), dpos.transpose(0, 1).reshape(T, C), mag)


# ---- the dropout mask of csrc/ctts_common.h in numpy uint64 arithmetic masked to 32 bits
_M32 = np.uint64(0xFFFFFFFF)
_G = np.uint64(0x9E3779B1)


def ctts_mix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def ctts_drop_key(seed_u64, offset):
    s = int(seed_u64) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)
    k = ctts_mix32(lo ^ ((np.uint64(int(offset) & 0xFFFFFFFF) * _G) & _M32))
    return ctts_mix32((k + hi) & _M32)


def attention_keep_mask(seed_u64, drop_offset, p, B, H, T):
    """bool [B,H,T,T]: element (b, head, i, j) has the index ((b*H + head)*T + i)*T + j (wrapping at 2^32) and is kept iff
    mix32(idx * 0x9E3779B1 + key) >= ceil(p * 2^24) << 8, p taken as a float32"""
    key = ctts_drop_key(seed_u64, drop_offset)
    idx = np.arange(B * H * T * T, dtype=np.uint64) & _M32
    h = ctts_mix32((idx * _G + key) & _M32)
    thr = np.uint64(int(np.ceil(float(np.float32(p)) * 16777216.0)) << 8)
    return torch.from_numpy((h >= thr).reshape(B, H, T, T))


# ---- the error measure
def slice_error_table(kernel, ref64, mag, lens, H, rows_last=False):
    """[B,H] table of max|kernel - ref64| / max(mag) over the valid rows of every (utterance, head) slice.  Tensors are [B,T,H*dh]
    (or [T,H*dh]: one utterance), with rows_last=True [B,H,T].  A slice without a valid row counts 0; a slice whose magnitude is
    exactly 0 has an exact result and counts 0 only if the kernel returned exactly that, else inf."""
    kernel, ref64, mag = (torch.as_tensor(t).detach().cpu().double() for t in (kernel, ref64, mag))
    if kernel.dim() == 2:
        kernel, ref64, mag = kernel[None], ref64[None], mag[None]
    if rows_last:
        kernel, ref64, mag = (t[..., None] for t in (kernel, ref64, mag))            # [B,H,T,1]
    else:
        kernel, ref64, mag = (_heads(t, H) for t in (kernel, ref64, mag))            # [B,H,T,dh]
    B, _, T, _ = ref64.shape
    assert kernel.shape == ref64.shape == mag.shape, (kernel.shape, ref64.shape, mag.shape)
    L = [T] * B if lens is None else [min(int(n), T) for n in lens]
    table = torch.zeros(B, H, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            if L[b] == 0:
                continue
            err = (kernel[b, h, :L[b]] - ref64[b, h, :L[b]]).abs().max().item()
            m = mag[b, h, :L[b]].max().item()
            if not err <= float("inf"):                   # NaN
                table[b, h] = float("inf")
            elif m > 0:
                table[b, h] = err / m
            else:
                table[b, h] = 0.0 if err == 0.0 else float("inf")
    return table


def slice_errors(kernel, ref64, mag, lens, H, rows_last=False):
    """the maximum of slice_error_table"""
    return slice_error_table(kernel, ref64, mag, lens, H, rows_last).max().item()


def fs2_parts(r):
    """Fs2 -> {part: tensor}"""
    return {n: getattr(r, n) for n in FS2_PARTS}


def rel_parts(r):
    """Rel -> {part: tensor} with dkv taken apart"""
    C = r.out.shape[-1]
    return {"out": r.out, "lse": r.lse, "dqu": r.dqu, "dqv": r.dqv, "dk": r.dkv[..., :C], "dv": r.dkv[..., C:], "dpos": r.dpos}


def part_errors(got, ref64_parts, mag, lens, H):
    """{part: slice_errors} for every part present in `got`"""
    return {n: slice_errors(t, ref64_parts[n], mag[n], None if n == "dpos" else lens, H, rows_last=(n == "lse")) for n, t in got.items()}
