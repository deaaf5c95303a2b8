"""float64 numpy restatement of fast Griffin-Lim (Perraudin, Balazs, Sondergaard 2013: the momentum of librosa / torchaudio) on
griffinlim_restate.transform / inverse, with the kernel's zero-magnitude rule, and an integer restatement of the device phase generator
of csrc/griffinlim.hip (ctts_mix32 chained over seed, b, f, k): the oracles of tests/test_fastgl_*.py.

One iteration, with X the rebuilt spectrum (the transform of the current signal), T the previous one (zero before the first):
    A = X - momentum / (1 + momentum) T,   T <- X,   signal <- inverse(magnitude, angle(A))
angle(0) = 0, so a bin with |A| = 0 becomes (magnitude, 0) - the kernel's rule, not librosa's A / (|A| + 1e-16)."""
import numpy as np

import griffinlim_restate as R


def griffin_lim(mag, angles, n_iters, momentum=0.99):
    """(mag, angles) [B,513,F] -> signal [B, 256 (F - 1)] after n_iters momentum iterations, float64"""
    mag = np.asarray(mag, dtype=np.float64)
    coef = momentum / (1.0 + momentum)
    signal = R.inverse(mag, angles)[:, 0]
    prev = np.zeros(mag.shape, dtype=np.complex128)
    for _ in range(n_iters):
        m, p = R.transform(signal)
        X = m * np.exp(1j * p)
        A = X - coef * prev
        prev = X
        signal = R.inverse(mag, np.angle(A))[:, 0]
    return signal


def spectral_convergence(signal, mag):
    """|| |STFT(signal)| - mag || / || mag ||"""
    m, _ = R.transform(signal)
    return R.rel_l2(m, np.asarray(mag, dtype=np.float64))


def stock_griffin_lim(stock, mag, angles, n_iters, momentum=0.99):
    """the same loop at float32 on stock torch ops (griffinlim_restate.StockSTFT, tensors on its device): the measure of the
    algorithm's own float32 drift on a given input"""
    import torch
    coef = momentum / (1.0 + momentum)
    signal = stock.inverse(mag, angles)[:, 0]
    pr = pi = None
    for _ in range(n_iters):
        m, p = stock.transform(signal)
        xr, xi = m * torch.cos(p), m * torch.sin(p)
        ar, ai = (xr, xi) if pr is None else (xr - coef * pr, xi - coef * pi)
        pr, pi = xr, xi
        signal = stock.inverse(mag, torch.atan2(ai, ar))[:, 0]
    return signal


# ---- the device phase generator: theta(seed, b, k, f) = 2 pi u, u = (h >> 8) 2^-24
_M32 = np.uint64(0xFFFFFFFF)
_G = np.uint64(0x9E3779B1)
_SITE = 0x474C5048


def _mix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def device_phase_u(seed, b, F, nbins=R.NB):
    """u [513, F] in [0, 1) of utterance b under `seed` (any Python int, taken modulo 2^64), float64 (exact: 24 bits)"""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)
    key = _mix32(lo ^ ((np.uint64(_SITE) * _G) & _M32))
    key = _mix32((key + hi) & _M32)
    kb = _mix32((key + np.uint64(b) * _G) & _M32)
    f = np.arange(F, dtype=np.uint64)
    fkey = _mix32((kb + f * _G) & _M32)                      # [F]
    k = np.arange(nbins, dtype=np.uint64)
    h = _mix32((fkey[None, :] + k[:, None] * _G) & _M32)    # [513, F]
    return (h >> np.uint64(8)).astype(np.float64) / 16777216.0


def device_phase(seed, B, F):
    """theta [B, 513, F] = 2 pi u, float64"""
    return np.stack([2.0 * np.pi * device_phase_u(seed, b, F) for b in range(B)])
