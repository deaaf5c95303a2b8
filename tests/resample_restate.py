"""Float64 restatement of the resampler and the peak normalisation (ctts_amd.resample, csrc/resample.hip), written from the definition
and sharing no code with the package:

    g = gcd(a, b), L = b / g, M = a / g, q = max(L, M), half = zeros q
    h[i] = L (rolloff / q) sinc(rolloff (i - half) / q) kaiser(2 half + 1, beta)[i]
    y[n] = sum_k h[n M + half - k L] x[k],   0 <= n < ceil(len L / M)

`resample_direct` is the double loop itself, `resample` the same sum gathered per output (vectorised, also returns sum |h x| and the
number of terms for the error bound), `resample_f32` the float32 evaluation with sequential accumulation in tap order that the tests
print next to the kernel's error.  `peak_normalize` is vctk.py:32-36 in numpy on a float32 array."""
import math

import numpy as np

PRESETS = {"kaiser_best": (64, 14.769656459379492, 0.9475937167399596), "kaiser_fast": (16, 8.555504641634386, 0.85)}
RATIOS = [(48000, 22050), (44100, 22050), (22050, 16000), (22050, 48000), (16000, 22050), (24000, 22050), (22050, 44100), (22050, 24000)]


def design(a, b, zeros=64, beta=PRESETS["kaiser_best"][1], rolloff=PRESETS["kaiser_best"][2]):
    """-> (L, M, half, h float64)"""
    g = math.gcd(a, b)
    L, M = b // g, a // g
    q = max(L, M)
    half = zeros * q
    i = np.arange(2 * half + 1, dtype=np.float64)
    h = L * (rolloff / q) * np.sinc(rolloff * (i - half) / q) * np.kaiser(2 * half + 1, beta)
    return L, M, half, h


def out_len(n, L, M):
    return -(-n * L // M)


def resample_direct(x, h, L, M):
    """the definition, term by term (small inputs only)"""
    half = (len(h) - 1) // 2
    y = np.zeros(out_len(len(x), L, M), dtype=np.float64)
    for n in range(len(y)):
        for k in range(len(x)):
            i = n * M + half - k * L
            if 0 <= i < len(h):
                y[n] += h[i] * x[k]
    return y


def _gather(x, h, L, M):
    """per output n the products h[n M + half - k L] x[k] over the taps that exist, as a [n_out, J] matrix (zeros where no tap), in
    order of increasing tap index j = k_hi - k"""
    half = (len(h) - 1) // 2
    n = np.arange(out_len(len(x), L, M), dtype=np.int64)
    t = n * M + half
    k_hi, r = t // L, t % L
    J = -(-len(h) // L)
    j = np.arange(J, dtype=np.int64)
    hi = r[:, None] + j[None, :] * L
    k = k_hi[:, None] - j[None, :]
    ok = (hi < len(h)) & (k >= 0) & (k < len(x))
    hv = np.where(ok, h[np.minimum(hi, len(h) - 1)], 0)
    xv = np.where(ok, x[np.clip(k, 0, len(x) - 1)], 0)
    return hv, xv, ok


def resample(x, h, L, M):
    """-> (y float64, sum_k |h x| per output, number of terms per output)"""
    hv, xv, ok = _gather(np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64), L, M)
    p = hv * xv
    return p.sum(1), np.abs(p).sum(1), ok.sum(1)


def resample_f32(x, h, L, M):
    """float32 taps, float32 products added one at a time in tap order (no fused multiply-add)"""
    hv, xv, _ = _gather(np.asarray(x, dtype=np.float32), np.asarray(h, dtype=np.float64).astype(np.float32), L, M)
    acc = np.zeros(hv.shape[0], dtype=np.float32)
    for j in range(hv.shape[1]):
        acc = acc + hv[:, j] * xv[:, j]
    return acc


def bank(h, L, T=None):
    """bank[r][j] = float32(h)[r + j L], zero beyond the end; T = ceil(len(h) / L) unless a wider one is asked for"""
    h32 = np.asarray(h, dtype=np.float64).astype(np.float32)
    T = T or -(-len(h32) // L)
    out = np.zeros((L, T), dtype=np.float32)
    for r in range(L):
        col = h32[r::L]
        out[r, :len(col)] = col
    return out


def peak_normalize(x, max_wav_value=32768.0):
    """vctk.py:32-36 on a float32 array -> (v float32 = x / max|x| * max_wav_value, its int16 cast saturated, q / 32768 float32).
    Where v == +32768 the reference's astype(np.int16) wraps; `wraps` marks those samples."""
    x = np.asarray(x, dtype=np.float32)
    v = x / np.max(np.abs(x)) * max_wav_value
    assert v.dtype == np.float32
    wraps = v >= 32768.0
    q = np.clip(np.trunc(v), -32768, 32767).astype(np.int16)
    ref = np.where(wraps, np.int16(-32768), np.trunc(np.where(wraps, 0, v)).astype(np.int16))      # what the reference writes
    return v, q, q.astype(np.float32) / np.float32(32768.0), ref, wraps
