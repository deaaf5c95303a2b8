"""Audio resampling and peak normalisation on the device (csrc/resample.hip): what `librosa.load(path, sampling_rate)` does to every file
the reference reads (preprocessor.py:364, :460, vctk.py:31 - for VCTK a 48 kHz -> 22.05 kHz band-limited resample) and what
`prepare_align` does next (vctk.py:32-36: divide by the peak, scale by max_wav_value, cast to int16).  The same primitive serves the
other end of the pipeline: the vocoders produce 22.05 kHz audio, callers may want 16 / 24 / 44.1 / 48 kHz.

  resample_filter   the windowed-sinc prototype, designed on the host in float64 (no GPU needed)
  resample          ragged, batched exact-phase polyphase filtering with that prototype
  peak_normalize    peak normalisation and 16-bit quantisation, saturating

The filter.  For orig_sr = a, target_sr = b: g = gcd(a, b), L = b / g (up), M = a / g (down), q = max(L, M), half = zeros q, and
    h[i] = L (rolloff / q) sinc(rolloff (i - half) / q) kaiser(2 half + 1, beta)[i],     0 <= i <= 2 half     (np.sinc, np.kaiser)
    y[n] = sum_k h[n M + half - k L] x[k],     0 <= n < ceil(len L / M),     x[k] = 0 outside [0, len)
which is scipy.signal.resample_poly(x, L, M, window=h / L, padtype="constant").  h is rounded once to float32 for the kernel.
"kaiser_best" (zeros 64, beta 14.769656459379492, rolloff 0.9475937167399596) carries the published constants of the filter librosa
0.7.2's `load` uses by default, "kaiser_fast" (16, 8.555504641634386, 0.85) those of its fast variant.  PARITY with librosa / resampy
is UNPINNED: neither is installed where this project is built, and resampy interpolates a table of the filter where this evaluates every
phase exactly.  The kernel is pinned against the float64 statement above only.

Lengths are device tensors (clamped by the kernels) or host sequences (checked here); nothing synchronises.  CPU tensors raise: there is
no CPU path.
"""
import math

import numpy as np
import torch

from . import kernels as K
from ._lib import CttsError
from .audio import _lens_arg

PRESETS = {
    "kaiser_best": {"zeros": 64, "beta": 14.769656459379492, "rolloff": 0.9475937167399596},
    "kaiser_fast": {"zeros": 16, "beta": 8.555504641634386, "rolloff": 0.85},
}
MAX_ZEROS = 64
_BANKS = {}


def _design(orig_sr, target_sr, quality, kw):
    """-> (L, M, zeros, beta, rolloff), checked"""
    if int(orig_sr) != orig_sr or int(target_sr) != target_sr or int(orig_sr) < 1 or int(target_sr) < 1:
        raise ValueError(f"resample: sampling rates must be positive integers, got {orig_sr} -> {target_sr}")
    a, b = int(orig_sr), int(target_sr)
    if quality not in PRESETS:
        raise ValueError(f"resample: quality {quality!r}: expected one of {sorted(PRESETS)}")
    extra = set(kw) - {"zeros", "beta", "rolloff"}
    if extra:
        raise TypeError(f"resample: unexpected filter arguments {sorted(extra)}")
    p = dict(PRESETS[quality], **kw)
    zeros, beta, rolloff = p["zeros"], float(p["beta"]), float(p["rolloff"])
    if int(zeros) != zeros or not 1 <= int(zeros) <= MAX_ZEROS:
        raise ValueError(f"resample: zeros must be an integer in [1, {MAX_ZEROS}], got {zeros}")
    if not (beta >= 0.0 and math.isfinite(beta)) or not 0.0 < rolloff <= 1.0:
        raise ValueError(f"resample: need beta >= 0 and 0 < rolloff <= 1, got {beta} / {rolloff}")
    g = math.gcd(a, b)
    L, M = b // g, a // g
    if max(L, M) > K.RESAMPLE_MAX_RATIO_TERM:
        raise ValueError(f"resample: {a} -> {b} reduces to {L}/{M}; both terms must be <= {K.RESAMPLE_MAX_RATIO_TERM}")
    return L, M, int(zeros), beta, rolloff


def phase_taps(L, half):
    """T: coefficients per phase of the bank handed to the kernel - ceil((2 half + 1) / L), rounded up to the kernel's granule of 8"""
    g = K.RESAMPLE_TAP_GRANULE
    return (-(-(2 * half + 1) // L) + g - 1) // g * g


def resample_filter(orig_sr, target_sr, quality="kaiser_best", **kw):
    """-> (L, M, h): the reduced ratio and the float64 prototype of 2 zeros max(L, M) + 1 taps (module docstring).  Host only.
    Explicit zeros= / beta= / rolloff= override the preset.  L == M gives h = [1.0]."""
    L, M, zeros, beta, rolloff = _design(orig_sr, target_sr, quality, kw)
    if L == M:
        return L, M, np.ones(1, dtype=np.float64)
    q = max(L, M)
    half = zeros * q
    if phase_taps(L, half) > K.RESAMPLE_MAX_PHASE_TAPS:
        raise ValueError(f"resample: {L}/{M} with {zeros} zero crossings needs {phase_taps(L, half)} taps per phase, more than "
                         f"{K.RESAMPLE_MAX_PHASE_TAPS}")
    i = np.arange(2 * half + 1, dtype=np.float64)
    h = L * (rolloff / q) * np.sinc(rolloff * (i - half) / q) * np.kaiser(2 * half + 1, beta)
    return L, M, h


def polyphase_bank(h, L):
    """float32 [L, T]: bank[r][j] = float32(h)[r + j L], zero beyond the last tap"""
    h32 = np.asarray(h, dtype=np.float64).astype(np.float32)
    T = phase_taps(L, (len(h32) - 1) // 2)
    flat = np.zeros(L * T, dtype=np.float32)
    flat[:len(h32)] = h32
    return np.ascontiguousarray(flat.reshape(T, L).T)


def _device_bank(orig_sr, target_sr, quality, kw, dev):
    L, M, zeros, beta, rolloff = _design(orig_sr, target_sr, quality, kw)
    if L == M:
        return L, M, 0, None
    key = (L, M, zeros, beta, rolloff, str(dev))
    if key not in _BANKS:
        _, _, h = resample_filter(orig_sr, target_sr, quality, **kw)
        _BANKS[key] = torch.from_numpy(polyphase_bank(h, L)).to(dev)
    return L, M, zeros * max(L, M), _BANKS[key]


def _batch_arg(wav, what):
    if not torch.is_tensor(wav) or not wav.is_cuda:
        raise CttsError(f"{what} computes on the MI355X: pass device tensors - no CPU fallback exists")
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise CttsError(f"{what}: expected a non-empty [B, N] tensor, got {tuple(wav.shape)}")
    if wav.shape[0] > 65535:
        raise CttsError(f"{what}: at most 65535 utterances per call, got {wav.shape[0]}")
    return wav.float().contiguous()


def output_length(n, L, M):
    return (int(n) * L + M - 1) // M


def resample(wav, lens, orig_sr, target_sr, quality="kaiser_best", **kw):
    """wav [B,N] (device), lens [B] samples (host sequence, checked: 0 <= len <= N; device tensor, clamped by the kernel; None: N) ->
    (out [B, ceil(N L / M)] float32, out_lens int32 [B] = ceil(lens L / M)) on the device.  Row b holds its utterance resampled from
    orig_sr to target_sr as if it had been alone (samples at and beyond lens[b] are never read), then exact zeros.  Equal rates copy."""
    wav = _batch_arg(wav, "resample")
    B, N = wav.shape
    L, M, half, bank = _device_bank(orig_sr, target_sr, quality, kw, wav.device)
    if lens is None:
        lens = [N] * B
    lens = _lens_arg(lens, B, 0, N, "resample lens", wav.device)
    return K.resample(wav, lens, bank, L, M, half)


def peak_normalize(wav, lens, max_wav_value=32768.0, return_int16=False):
    """`prepare_align`'s `wav / max(abs(wav)) * max_wav_value` and `.astype(np.int16)` (vctk.py:32-36) on a ragged batch.
    wav [B,N] (device), lens as in `resample` -> (out [B,N] float32, valid int32 [B]) and, with return_int16, the int16 values [B,N] as
    a third result.  out = q / 32768 with q = trunc(v) saturated to [-32768, 32767]: what reading the written 16-bit file back gives; 0
    at and beyond lens[b].  The peak is taken over the utterance's own samples.  Where the reference's cast of exactly +32768.0 wraps to
    -32768 (undefined in C), this saturates to 32767.  An all-zero utterance gives zeros and valid = 0 (the reference divides by zero)."""
    wav = _batch_arg(wav, "peak_normalize")
    B, N = wav.shape
    if lens is None:
        lens = [N] * B
    lens = _lens_arg(lens, B, 0, N, "peak_normalize lens", wav.device)
    out, q16, _, valid = K.peak_normalize(wav, lens, max_wav_value, return_int16)
    return (out, valid, q16) if return_int16 else (out, valid)
