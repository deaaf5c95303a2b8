"""The waveform metrics of ctts_amd.metrics restated in numpy: STOI / ESTOI, SI-SDR and the multi-resolution STFT distances exactly as the
module docstring defines them.  Every function takes `dtype`: np.float64 is the contract the kernels are tested against; np.float32 is
the same chain evaluated in stock float32 (float32 arrays, scipy.fft keeps float32), the yardstick of tests/test_wavmetrics_gpu.py.
The float32 evaluation takes the keep decision of the silent-frame step from the float64 one, so that it measures rounding, not a
flipped frame.  Pinned by tests/test_wavmetrics_restate_cpu.py.  PARITY with pystoi is UNPINNED (not installed; its resampler differs)."""
import numpy as np
import scipy.fft

FS, FRAME, HOP, NFFT, BANDS, SEG = 10000, 256, 128, 512, 15, 30
BETA_DB, RANGE_DB = -15.0, 40.0
EPS = 2.0 ** -52
MR_DEFAULT = ((512, 50, 240), (1024, 120, 600), (2048, 240, 1200))
MR_CLAMP = 1e-7


def window():
    return np.hanning(FRAME + 2)[1:-1]


def band_edges():
    """[(lo_j, hi_j)]: the bins nearest to 150 * 2^((2j -+ 1) / 6) Hz on the grid k * FS / NFFT"""
    grid = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    j = np.arange(BANDS)
    lo = [int(np.argmin(np.abs(grid - 150.0 * 2.0 ** ((2 * v - 1) / 6.0)))) for v in j]
    hi = [int(np.argmin(np.abs(grid - 150.0 * 2.0 ** ((2 * v + 1) / 6.0)))) for v in j]
    return list(zip(lo, hi))


def n_frames(n, win=FRAME, hop=HOP):
    return (n - win) // hop + 1 if n >= win else 0


def _frames(x, win, hop):
    F = n_frames(len(x), win, hop)
    return x[hop * np.arange(F)[:, None] + np.arange(win)[None, :]] if F else np.zeros((0, win), dtype=x.dtype)


def frame_energies_db(x):
    """e_i of the silent-frame step, float64"""
    fr = _frames(np.asarray(x, dtype=np.float64), FRAME, HOP) * window()
    return 20.0 * np.log10(np.sqrt(np.sum(fr * fr, axis=1)) + EPS)


def keep_mask(x):
    e = frame_energies_db(x)
    return e > (e.max() - RANGE_DB) if len(e) else np.zeros(0, dtype=bool)


def threshold_margin_db(x):
    """the smallest | e_i - (max e - 40) | over the frames: how far the nearest frame is from changing sides"""
    e = frame_energies_db(x)
    return float(np.min(np.abs(e - (e.max() - RANGE_DB)))) if len(e) else np.inf


def _compact(x, keep, w):
    fr = (_frames(x, FRAME, HOP) * w)[keep]
    K = len(fr)
    out = np.zeros(HOP * (K - 1) + FRAME if K else 0, dtype=x.dtype)
    for m in range(K):                                              # kept order
        out[HOP * m:HOP * m + FRAME] += fr[m]
    return out


def band_amplitudes(x, keep, dtype=np.float64):
    """[15, K]: third-octave band amplitudes of the frames of the compacted signal"""
    w = window().astype(dtype)
    xc = _compact(np.asarray(x, dtype=dtype), keep, w)
    spec = scipy.fft.rfft(_frames(xc, FRAME, HOP) * w, n=NFFT, axis=1)
    p = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
    return np.stack([np.sqrt(np.sum(p[:, lo:hi], axis=1)) for lo, hi in band_edges()], axis=0).astype(dtype)


def _segments(a):
    S = a.shape[1] - SEG + 1
    return np.stack([a[:, s:s + SEG] for s in range(S)], axis=0)    # [S, 15, 30]


def stoi(x, y, dtype=np.float64):
    """-> dict(stoi, estoi, frames, kept, segments) of one pair at 10 kHz"""
    x, y = np.asarray(x), np.asarray(y)
    assert x.shape == y.shape and x.ndim == 1
    F = n_frames(len(x))
    nan = float("nan")
    if F == 0:
        return {"stoi": nan, "estoi": nan, "frames": 0, "kept": 0, "segments": 0}
    keep = keep_mask(x)
    K = int(keep.sum())
    silent = float(np.max(np.sum((_frames(x.astype(np.float64), FRAME, HOP) * window()) ** 2, axis=1))) == 0.0
    if K < SEG or silent:
        return {"stoi": nan, "estoi": nan, "frames": F, "kept": K, "segments": 0}
    eps = dtype(EPS)
    X, Y = _segments(band_amplitudes(x, keep, dtype)), _segments(band_amplitudes(y, keep, dtype))
    S = X.shape[0]
    # STOI
    alpha = np.linalg.norm(X, axis=2, keepdims=True) / (np.linalg.norm(Y, axis=2, keepdims=True) + eps)
    Yp = np.minimum(alpha * Y, X * dtype(1.0 + 10.0 ** (-BETA_DB / 20.0)))
    Xc, Yc = X - X.mean(axis=2, keepdims=True), Yp - Yp.mean(axis=2, keepdims=True)
    Xc = Xc / (np.linalg.norm(Xc, axis=2, keepdims=True) + eps)
    Yc = Yc / (np.linalg.norm(Yc, axis=2, keepdims=True) + eps)
    d = float(np.sum(Xc * Yc, dtype=dtype) / dtype(BANDS * S))
    # ESTOI
    def rowcol(a):
        a = a - a.mean(axis=2, keepdims=True)
        a = a / (np.linalg.norm(a, axis=2, keepdims=True) + eps)
        a = a - a.mean(axis=1, keepdims=True)
        return a / (np.linalg.norm(a, axis=1, keepdims=True) + eps)
    e = float(np.sum(rowcol(X) * rowcol(Y) / dtype(SEG), dtype=dtype) / dtype(S))
    return {"stoi": d, "estoi": e, "frames": F, "kept": K, "segments": S}


def si_sdr(x, y, dtype=np.float64):
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    if len(x) == 0:
        return float("nan")
    xc, yc = x - x.mean(dtype=dtype), y - y.mean(dtype=dtype)
    sxx = np.dot(xc, xc)
    if sxx == 0:
        return float("nan")
    t = (np.dot(yc, xc) / sxx) * xc
    r = yc - t
    tt, rr = float(np.dot(t, t)), float(np.dot(r, r))
    if rr == 0.0:
        return float("inf") if tt > 0.0 else float("nan")
    return float(10.0 * np.log10(tt / rr))


def mr_window(win, dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / float(win))).astype(dtype)


def stft_distance(x, y, n_fft, hop, win, dtype=np.float64):
    """-> (sc, log_mag, lsd_db, frames) of one pair at one resolution"""
    assert n_fft in (512, 1024, 2048) and 1 <= win <= n_fft and hop >= 1
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    F = n_frames(len(x), win, hop)
    if F == 0:
        return float("nan"), float("nan"), float("nan"), 0
    w = mr_window(win, dtype)

    def mag(v):
        s = scipy.fft.rfft(_frames(v, win, hop) * w, n=n_fft, axis=1)
        return np.sqrt(np.maximum(s.real * s.real + s.imag * s.imag, dtype(MR_CLAMP))).astype(dtype)
    mx, my = mag(x), mag(y)
    sc = np.sqrt(np.sum((mx - my) ** 2, dtype=dtype)) / np.sqrt(np.sum(mx * mx, dtype=dtype))
    log_mag = np.mean(np.abs(np.log(mx) - np.log(my)), dtype=dtype)
    lsd = np.mean(np.sqrt(np.mean((dtype(20.0) * np.log10(mx) - dtype(20.0) * np.log10(my)) ** 2, axis=1, dtype=dtype)), dtype=dtype)
    return float(sc), float(log_mag), float(lsd), F


def mr_stft_distance(x, y, resolutions=MR_DEFAULT, dtype=np.float64):
    """-> dict of [R] arrays: sc, log_mag, lsd_db, frames"""
    r = [stft_distance(x, y, n, h, w, dtype) for n, h, w in resolutions]
    return {"sc": np.array([v[0] for v in r]), "log_mag": np.array([v[1] for v in r]), "lsd_db": np.array([v[2] for v in r]),
            "frames": np.array([v[3] for v in r], dtype=np.int32)}
