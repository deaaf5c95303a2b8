"""Seeded input families of tests/test_attention_gpu.py, shared with tests/test_attention_restate_cpu.py so that the CPU conditioning
test sees exactly the inputs the kernels are run on.  All of them start from a uniform [-1, 1] base.

    flat             q = 0: P = 1/L exactly, lse = ln L, out = mean of v over the valid keys
    soft             the base as it is (scores of standard deviation ~0.3)
    peaked           q *= 24: mean largest probability ~0.8
    huge             q *= 72: largest probability ~0.93, exp2 underflow for most keys, large lse
    ramp_up          k[b,j,:] += j/dh, q += 1: scores rise with the key index, the running max moves in every key tile
    ramp_down        k[b,j,:] -= j/dh, q += 1: the max is in the first tile, later tiles only add tails
    content_peaked   (rel) qu *= 24
    position_peaked  (rel) qv *= 24: the position band decides every row"""
import torch

FS2_REGIMES = ("flat", "soft", "peaked", "huge", "ramp_up", "ramp_down")
REL_REGIMES = ("soft", "content_peaked", "position_peaked", "ramp_up", "ramp_down")
EDGE_T = 97
EDGE_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97)          # every edge of the 32-wide query / key tiles, one below, one above
FS2_HEADS = (8, 4, 2)                                            # C = 256: d_head 32, 64, 128
REL_T = (1, 2, 31, 32, 33, 63, 64, 65, 97)
REL_HC = ((8, 256), (2, 128), (1, 128))                          # d_head 32, 64, 128


def base(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def _ramp(T, dh):
    return (torch.arange(T, dtype=torch.float32) / dh)[None, :, None]


def fs2_inputs(regime, B, T, H, C=256, seed=0):
    """-> (qkv [B,T,3C], dout [B,T,C]) float32"""
    qkv = base(B, T, 3 * C, seed=1000 + seed)
    dout = base(B, T, C, seed=2000 + seed)
    q, k = qkv[..., :C], qkv[..., C:2 * C]
    if regime == "flat":
        q.zero_()
    elif regime == "peaked":
        q *= 24
    elif regime == "huge":
        q *= 72
    elif regime in ("ramp_up", "ramp_down"):
        k += _ramp(T, C // H) * (1 if regime == "ramp_up" else -1)
        q += 1
    else:
        assert regime == "soft", regime
    return qkv, dout


def rel_inputs(regime, B, T, H, C, seed=0):
    """-> (qu, qv [B,T,C], kv [B,T,2C], pos [T,C], dout [B,T,C]) float32"""
    qu, qv, kv = base(B, T, C, seed=3000 + seed), base(B, T, C, seed=3100 + seed), base(B, T, 2 * C, seed=3200 + seed)
    pos, dout = base(T, C, seed=3300 + seed), base(B, T, C, seed=3400 + seed)
    if regime == "content_peaked":
        qu *= 24
    elif regime == "position_peaked":
        qv *= 24
    elif regime in ("ramp_up", "ramp_down"):
        kv[..., :C] += _ramp(T, C // H) * (1 if regime == "ramp_up" else -1)
        qu += 1
    else:
        assert regime == "soft", regime
    return qu, qv, kv, pos, dout
