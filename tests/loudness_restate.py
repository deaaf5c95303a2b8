"""float64 restatement of ITU-R BS.1770-4 gated loudness as `pyloudnorm.Meter(rate)` implements it, for mono signals - the definition
the loudness kernels (csrc/loudness.hip, ctts_amd.loudness) are tested against.  numpy / scipy only; `scipy.signal.lfilter` is the
filter.  pyloudnorm itself is not installed where this project is built, so parity with it is unpinned: tests/test_loudness_restate_cpu.py
pins this file against the standard's own filter table and conformance points instead.

K-weighting: two RBJ biquads designed per sampling rate, a high shelf (+4 dB, Q = 1/sqrt 2, 1500 Hz) and a high pass (Q = 0.5, 38 Hz).
Blocks of T_g seconds every 0.25 T_g; z_j = sum y^2 / (T_g rate) over samples [int(T_g (j 0.25) rate), min(int(T_g (j 0.25 + 1) rate), N)),
always divided by the whole block; l_j = -0.691 + 10 log10 z_j; absolute gate -70, relative gate 10 LU under the loudness of the blocks
that pass the absolute one.  The short-term curve is the same construction with T_g = 3 s at the same 0.1 s hop (step = 0.1 / 3)."""
import math

import numpy as np
from scipy.signal import lfilter

T_MOMENTARY, STEP_MOMENTARY = 0.4, 0.25
T_SHORT_TERM, STEP_SHORT_TERM = 3.0, 0.1 / 3.0
ABSOLUTE_GATE = -70.0


def high_shelf(rate, gain_db=4.0, q=1.0 / math.sqrt(2.0), fc=1500.0):
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * math.pi * fc / rate
    alpha = math.sin(w0) / (2.0 * q)
    c, r = math.cos(w0), 2.0 * math.sqrt(A) * alpha
    b = np.array([A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r)], dtype=np.float64)
    a = np.array([(A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r], dtype=np.float64)
    return b / a[0], a / a[0]


def high_pass(rate, q=0.5, fc=38.0):
    w0 = 2.0 * math.pi * fc / rate
    alpha = math.sin(w0) / (2.0 * q)
    c = math.cos(w0)
    b = np.array([(1 + c) / 2, -(1 + c), (1 + c) / 2], dtype=np.float64)
    a = np.array([1 + alpha, -2 * c, 1 - alpha], dtype=np.float64)
    return b / a[0], a / a[0]


def kweighting(rate):
    """-> ((b, a) of the shelf, (b, a) of the high pass), a[0] = 1, float64"""
    return high_shelf(rate), high_pass(rate)


def kweight(x, rate, dtype=np.float64):
    """the K-weighted signal; dtype=np.float32 evaluates the same chain on float32 arrays (what a stock float32 filter gives)"""
    y = np.asarray(x, dtype=dtype)
    for b, a in kweighting(rate):
        y = lfilter(b.astype(dtype), a.astype(dtype), y)
        assert y.dtype == dtype
    return y


def n_blocks(n, rate, t_g=T_MOMENTARY, step=STEP_MOMENTARY):
    return int(round((n / rate - t_g) / (t_g * step))) + 1


def block_bounds(j, rate, t_g=T_MOMENTARY, step=STEP_MOMENTARY):
    """[lo, hi) of block j before it is cut at the signal's end"""
    return int(t_g * (j * step) * rate), int(t_g * (j * step + 1) * rate)


def block_energies(x, rate, t_g=T_MOMENTARY, step=STEP_MOMENTARY, dtype=np.float64):
    """z_j of every block (float64 sums of the dtype-filtered signal)"""
    x = np.asarray(x)
    n = len(x)
    if n < t_g * rate:
        raise ValueError(f"{n} samples are shorter than one block of {t_g} s at {rate} Hz")
    y = kweight(x, rate, dtype).astype(np.float64)
    z = np.zeros(n_blocks(n, rate, t_g, step), dtype=np.float64)
    for j in range(len(z)):
        lo, hi = block_bounds(j, rate, t_g, step)
        z[j] = np.sum(np.square(y[lo:min(hi, n)])) / (t_g * rate)
    return z


def _lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def gate(z):
    """-> (integrated loudness, valid) from the block energies"""
    l = _lufs(z)
    first = z[l >= ABSOLUTE_GATE]
    if len(first) == 0:
        return -math.inf, 0
    gamma_r = -0.691 + 10.0 * math.log10(np.mean(first)) - 10.0
    second = z[(l > gamma_r) & (l > ABSOLUTE_GATE)]
    if len(second) == 0:
        return -math.inf, 0
    return -0.691 + 10.0 * math.log10(np.mean(second)), 1


def integrated_loudness(x, rate, dtype=np.float64):
    """-> (L in LUFS or -inf, valid)"""
    return gate(block_energies(x, rate, dtype=dtype))


def momentary(x, rate, dtype=np.float64):
    return _lufs(block_energies(x, rate, T_MOMENTARY, STEP_MOMENTARY, dtype))


def short_term(x, rate, dtype=np.float64):
    return _lufs(block_energies(x, rate, T_SHORT_TERM, STEP_SHORT_TERM, dtype))


def normalize(x, rate, target=-22.0, peak_limit=True):
    """-> (out float64, L, gain, valid): out = x gain with gain = 10^((target - L) / 20), divided by max |out| when that exceeds 1
    (audio/stft.py:230-231); an utterance no block of which passes the gates is returned unchanged with gain 1"""
    x = np.asarray(x, dtype=np.float64)
    L, valid = integrated_loudness(x, rate)
    if not valid:
        return x.copy(), L, 1.0, 0
    gain = 10.0 ** ((target - L) / 20.0)
    if peak_limit:
        peak = np.max(np.abs(x * gain))
        if peak > 1.0:
            gain = gain / peak
    return x * gain, L, gain, 1
