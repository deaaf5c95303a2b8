"""Loudness metering and normalisation on the device (csrc/loudness.hip): ITU-R BS.1770-4 gated loudness of mono utterances, what the
reference computes on the host with `pyloudnorm.Meter(rate).integrated_loudness` and `pyloudnorm.normalize.loudness` before feature
extraction (audio/stft.py:226-231, target -22 LUFS, divided by the peak when the result would clip).

  kweighting            the two K-weighting biquads for a sampling rate, float64 (no GPU needed)
  integrated_loudness   gated loudness of every utterance of a ragged batch
  loudness_curve        momentary (0.4 s) or short-term (3 s) loudness every 0.1 s
  normalize_loudness    the utterances brought to a target loudness, with the reference's peak guard

The definition (tests/loudness_restate.py states it in float64 with scipy).  K-weighting is a high shelf (RBJ, +4 dB, Q = 1/sqrt 2,
1500 Hz) followed by a high pass (RBJ, Q = 0.5, 38 Hz), designed for the rate.  Blocks of T_g = 0.4 s every 0.1 s; block j covers
samples [int(T_g (j 0.25) rate), min(int(T_g (j 0.25 + 1) rate), N)), z_j = sum y^2 / (T_g rate) - the whole block even where it was
cut at N - for j < int(round((N / rate - T_g) / (T_g 0.25))) + 1; l_j = -0.691 + 10 log10 z_j.  Absolute gate -70 LUFS; relative gate
10 LU below the loudness of the blocks above the absolute gate; L = -0.691 + 10 log10 of the mean z_j over the blocks above both.
PARITY with pyloudnorm is UNPINNED: it is not installed where this project is built.  The kernels are pinned against the float64
restatement, and that against the standard's filter table and conformance tones.

The block edges are evaluated here, on the host, by the very expressions above (in floating point int(0.4 * (3 * 0.25) * 22050) need
not be 6615), and handed to the kernels as integer tables, so the device cuts where the definition cuts.  Lengths are HOST integers
(the number of blocks follows from them); a device tensor of lengths is copied to the host first.  CPU tensors raise: there is no CPU
path.  Every result of an utterance is bit-identical whatever batch it is measured in."""
import math

import numpy as np
import torch

from . import kernels as K
from ._lib import CttsError

WINDOWS = {"momentary": (0.4, 0.25), "short_term": (3.0, 0.1 / 3.0)}     # T_g seconds, step as a fraction of T_g
_COEF = {}
_TABLES = {}


def _rate(rate):
    if int(rate) != rate or int(rate) < 1000:
        raise ValueError(f"loudness: the sampling rate must be an integer of at least 1000 Hz, got {rate}")
    return int(rate)


def kweighting(rate):
    """-> ((b, a) of the high shelf, (b, a) of the high pass): float64 arrays of three coefficients, a[0] = 1.  Host only."""
    rate = _rate(rate)
    A = 10.0 ** (4.0 / 40.0)
    w0 = 2.0 * math.pi * 1500.0 / rate
    alpha = math.sin(w0) / (2.0 * (1.0 / math.sqrt(2.0)))
    c, r = math.cos(w0), 2.0 * math.sqrt(A) * alpha
    b1 = np.array([A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r)], dtype=np.float64)
    a1 = np.array([(A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r], dtype=np.float64)
    w0 = 2.0 * math.pi * 38.0 / rate
    alpha = math.sin(w0) / (2.0 * 0.5)
    c = math.cos(w0)
    b2 = np.array([(1 + c) / 2, -(1 + c), (1 + c) / 2], dtype=np.float64)
    a2 = np.array([1 + alpha, -2 * c, 1 - alpha], dtype=np.float64)
    return (b1 / a1[0], a1 / a1[0]), (b2 / a2[0], a2 / a2[0])


def state_transition(rate):
    """4 x 4 float64 matrix that advances the cascade's state (z1, z2 of the shelf, z1, z2 of the high pass; transposed direct form II)
    by one sample of zero input"""
    (sb, sa), (hb, ha) = kweighting(rate)
    return np.array([[-sa[1], 1.0, 0.0, 0.0],
                     [-sa[2], 0.0, 0.0, 0.0],
                     [hb[1] - ha[1] * hb[0], 0.0, -ha[1], 1.0],
                     [hb[2] - ha[2] * hb[0], 0.0, -ha[2], 0.0]], dtype=np.float64)


def coefficient_words(rate):
    """the float64 buffer the kernels read (include/ctts.h): both biquads, then A^(chunk 16^l m) for l = 0 .. 4, m = 1 .. 16"""
    (sb, sa), (hb, ha) = kweighting(rate)
    n = K.loudness_limits()[1]
    out = np.zeros(n, dtype=np.float64)
    out[0:5] = [sb[0], sb[1], sb[2], sa[1], sa[2]]
    out[5:10] = [hb[0], hb[1], hb[2], ha[1], ha[2]]
    A, chunk = state_transition(rate), K.loudness_chunk()
    levels = (n - 16) // 256
    for l in range(levels):
        base = np.linalg.matrix_power(A, chunk * 16 ** l)
        p = np.eye(4)
        for m in range(16):
            p = base @ p
            out[16 + 16 * (16 * l + m):16 + 16 * (16 * l + m + 1)] = p.reshape(-1)
    return out


def _coef(rate, dev):
    key = (rate, str(dev))
    if key not in _COEF:
        _COEF[key] = torch.from_numpy(coefficient_words(rate)).to(dev)
    return _COEF[key]


def n_blocks(n, rate, window="momentary"):
    t_g, step = WINDOWS[window]
    return int(round((n / rate - t_g) / (t_g * step))) + 1


def block_tables(rate, window, n_samples):
    """-> (edges int32, chunk_seg int32, blocks int32 [J,2]) as numpy arrays for rows of up to n_samples samples (include/ctts.h,
    "Loudness on the device").  Everything is counted from sample 0, so the tables of a longer row extend those of a shorter one."""
    t_g, step = WINDOWS[window]
    chunk = K.loudness_chunk()
    slots, _, max_segs = K.loudness_limits()
    tile = 64 * chunk
    ntiles = (int(n_samples) + tile - 1) // tile
    J = max(1, n_blocks(ntiles * tile, rate, window))
    lo = [int(t_g * (j * step) * rate) for j in range(J)]
    hi = [int(t_g * (j * step + 1) * rate) for j in range(J)]
    # every start and end of ANY block that falls inside [0, hi[J-1]] is an edge, also those of blocks beyond J (in floating point
    # the end of block j need not be the start of block j + 1 / step): the cut of the time axis depends on the position alone
    every, j = {0}, 0
    while int(t_g * (j * step) * rate) <= hi[-1]:
        every |= {int(t_g * (j * step) * rate), int(t_g * (j * step + 1) * rate)}
        j += 1
    edges = np.array(sorted(e for e in every if e <= hi[-1]), dtype=np.int64)
    if J > max_segs or len(edges) - 1 > max_segs or edges[-1] >= 2 ** 31 - 1:
        raise ValueError(f"loudness: {n_samples} samples at {rate} Hz make {J} blocks / {len(edges) - 1} hop segments; the gate holds {max_segs}")
    starts = np.arange(ntiles * 64, dtype=np.int64) * chunk
    chunk_seg = np.searchsorted(edges, starts, side="right") - 1
    last = np.searchsorted(edges, (np.arange(ntiles, dtype=np.int64) + 1) * tile - 1, side="right") - 1
    if np.max(last - chunk_seg[::64]) + 1 > slots:
        raise ValueError(f"loudness: at {rate} Hz a tile of {tile} samples touches more than {slots} hop segments")
    blocks = np.stack([np.searchsorted(edges, lo), np.searchsorted(edges, hi)], axis=1)
    edges = np.concatenate([edges, [2 ** 31 - 1]])
    return edges.astype(np.int32), chunk_seg.astype(np.int32), np.ascontiguousarray(blocks.astype(np.int32))


def _tables(rate, window, N, dev):
    tile = 64 * K.loudness_chunk()
    key = (rate, window, (N + tile - 1) // tile, str(dev))
    if key not in _TABLES:
        _TABLES[key] = tuple(torch.from_numpy(t).to(dev) for t in block_tables(rate, window, N))
    return _TABLES[key]


def _batch(wav, lens, rate, window, what):
    if not torch.is_tensor(wav) or not wav.is_cuda:
        raise CttsError(f"{what} computes on the MI355X: pass device tensors - no CPU fallback exists")
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise CttsError(f"{what}: expected a non-empty [B, N] tensor, got {tuple(wav.shape)}")
    wav = wav.float().contiguous()
    B, N = wav.shape
    if lens is None:
        lens = [N] * B
    v = [int(n) for n in (lens.tolist() if torch.is_tensor(lens) else lens)]
    if len(v) != B:
        raise ValueError(f"{what}: {len(v)} lengths for a batch of {B}")
    if min(v) < 0 or max(v) > N:
        raise ValueError(f"{what}: lengths must lie in [0, {N}], got {min(v)} .. {max(v)}")
    t_g = WINDOWS[window][0]
    short = [i for i, n in enumerate(v) if n < t_g * rate]
    if short:
        raise ValueError(f"{what}: utterances {short} are shorter than one block of {t_g} s at {rate} Hz "
                         f"({[v[i] for i in short]} samples, {math.ceil(t_g * rate)} needed)")
    nb = [n_blocks(n, rate, window) for n in v]
    dev = wav.device
    return wav, torch.tensor(v, dtype=torch.int32).to(dev), torch.tensor(nb, dtype=torch.int32).to(dev), max(nb)


def _measure(wav, lens, rate, window, target, peak_limit, curve, what):
    rate = _rate(rate)
    if window not in WINDOWS:
        raise ValueError(f"{what}: window {window!r}: expected one of {sorted(WINDOWS)}")
    wav, lens_d, nb_d, nb_max = _batch(wav, lens, rate, window, what)
    N = wav.shape[1]
    edges, chunk_seg, blocks = _tables(rate, window, N, wav.device)
    hop_sums, peak = K.kweight_energy(wav, lens_d, _coef(rate, wav.device), edges, chunk_seg)
    loud, gain, valid, cur = K.loudness_gate(hop_sums, lens_d, nb_d, edges, chunk_seg, blocks, peak, N, WINDOWS[window][0] * rate, target,
                                             peak_limit, curve)
    return wav, lens_d, loud, gain, valid, (cur[:, :nb_max] if curve else None)


def integrated_loudness(wav, lens, rate):
    """wav [B,N] (device), lens [B] host ints (None: N) -> (loudness float64 [B] in LUFS, -inf where valid is 0; valid int32 [B]) on the
    device.  Raises ValueError naming the utterances shorter than 0.4 s."""
    _, _, loud, _, valid, _ = _measure(wav, lens, rate, "momentary", -22.0, False, False, "integrated_loudness")
    return loud, valid


def loudness_curve(wav, lens, rate, window="momentary"):
    """-> float64 [B, J] on the device: the loudness of every block of 0.4 s ("momentary") or 3 s ("short_term"), one every 0.1 s,
    J the block count of the longest utterance; -inf for a silent block and at and beyond an utterance's own block count"""
    return _measure(wav, lens, rate, window, -22.0, False, True, "loudness_curve")[5]


def normalize_loudness(wav, lens, rate, target=-22.0, peak_limit=True, out=None):
    """-> (wav_out float32 [B,N], loudness float64 [B], gain float32 [B], valid int32 [B]) on the device.  wav_out = wav * gain inside
    lens (one fp32 product), exact zeros beyond; gain = 10^((target - loudness) / 20), or 1 / max |wav| when peak_limit is set and the
    result would exceed 1 (audio/stft.py:230-231).  An utterance with valid = 0 (no block above the gates) is returned unchanged with
    gain 1.  `out` may be `wav` (float32, contiguous) for an in-place result."""
    if not math.isfinite(float(target)):
        raise ValueError(f"normalize_loudness: the target must be finite, got {target}")
    wav, lens_d, loud, gain, valid, _ = _measure(wav, lens, rate, "momentary", float(target), bool(peak_limit), False, "normalize_loudness")
    return K.apply_gain(wav, lens_d, gain, out), loud, gain, valid
