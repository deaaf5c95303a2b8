"""Independent model of the mel front end (TacotronSTFT.mel_spectrogram: reflect padding, centred periodic hann window, DFT, |X|,
energy, mel filterbank, log clamp) in plain numpy.  It imports nothing from the package: the filterbank comes in as an array
(tests/test_mel_basis_cpu.py owns the Slaney construction) and every other ingredient is written out here.

mel_frontend(..., dtype=np.float64) is the reference of tests/test_mel_kernels_gpu.py; dtype=np.float32 is the float32 TWIN: the
reference project's own formulation (a product with the windowed [2 * nbins, n_fft] DFT basis - the weight of its conv1d - then the
float32 filterbank product) carried in float32 on the CPU.  mel_frontend_scipy32 is a second float32 evaluation (scipy's float32 rFFT),
printed for information only.

Conventions shared with the kernels (their documented contract, not their code):
  F = 1 + N // hop frames per batch row; frame f holds the samples [f * hop - n_fft/2, f * hop + n_fft/2) of the waveform reflected
  about its first and its last sample (numpy / torch "reflect": the edge sample is not repeated);
  a ragged row b holds Nb = clamp(lens[b], n_fft/2 + 1, N) samples: the reflection happens at ITS last sample, it has
  Fb = min(F, 1 + Nb // hop) frames, and the remaining frames of the row repeat frame Fb - 1.
"""
import numpy as np

MISREADINGS = ("symmetric_window", "zero_padding", "frames_n_over_hop", "uncentred_window", "reflect_at_row_end", "energy_kept_bins")


def hann(win_length, periodic=True):
    """0.5 - 0.5 cos(2 pi n / D) in float64: D = win_length (periodic, scipy get_window(..., fftbins=True)) or win_length - 1"""
    n = np.arange(win_length, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (win_length if periodic else win_length - 1))


def analysis_window(n_fft, win_length, periodic=True, centred=True):
    """the window zero-padded to n_fft: (n_fft - win_length) // 2 zeros in front (centred) or none (the misreading)"""
    lpad = (n_fft - win_length) // 2 if centred else 0
    w = np.zeros(n_fft, dtype=np.float64)
    w[lpad:lpad + win_length] = hann(win_length, periodic)
    return w


def reflect_index(p, n):
    """index into a row of n samples for position p of the row reflected about sample 0 and about sample n - 1 (one reflection: |p| and
    p - (n - 1) stay below n - 1 for every frame position when n > n_fft / 2)"""
    p = np.abs(np.asarray(p, dtype=np.int64))
    return np.where(p >= n, 2 * (n - 1) - p, p)


def frame_counts(N, lens, n_fft, hop, B):
    """(F, Nb [B], Fb [B])"""
    F = 1 + N // hop
    if lens is None:
        nb = np.full(B, N, dtype=np.int64)
    else:
        nb = np.minimum(np.maximum(np.asarray(lens, dtype=np.int64), n_fft // 2 + 1), N)
    return F, nb, np.minimum(F, 1 + nb // hop)


def frame_matrix(y, lens, n_fft, hop, misread=None):
    """y [B, N] -> frames [B, F, n_fft] (a gather, exact in y's dtype)"""
    y = np.asarray(y)
    B, N = y.shape
    F, nb, fb = frame_counts(N, lens, n_fft, hop, B)
    if misread == "frames_n_over_hop":
        F = N // hop
        fb = np.minimum(fb, F)
    out = np.zeros((B, F, n_fft), dtype=y.dtype)
    for b in range(B):
        n_end = N if misread == "reflect_at_row_end" else int(nb[b])
        f = np.minimum(np.arange(F), fb[b] - 1)
        pos = f[:, None] * hop - n_fft // 2 + np.arange(n_fft)[None, :]
        if misread == "zero_padding":
            ok = (pos >= 0) & (pos < n_end)
            out[b] = np.where(ok, y[b][np.clip(pos, 0, n_end - 1)], 0)
        else:
            out[b] = y[b][reflect_index(pos, n_end)]
    return out


def dft_basis(n_fft, window):
    """[2 * nbins, n_fft] float64: rows [0, nbins) = cos(2 pi k n / n_fft) w[n], rows [nbins, 2 nbins) = -sin(...) w[n]"""
    nbins = n_fft // 2 + 1
    kn = (np.arange(nbins, dtype=np.int64)[:, None] * np.arange(n_fft, dtype=np.int64)[None, :]) % n_fft      # exact phase index
    ang = 2.0 * np.pi * kn.astype(np.float64) / n_fft
    return np.vstack([np.cos(ang), -np.sin(ang)]) * window[None, :]


def mel_frontend(y, lens, n_fft, hop, win_length, basis, clip=1e-5, dtype=np.float64, misread=None):
    """-> (mag [B, F, nbins], energy [B, F], mel_lin [B, n_mel, F], mel_log [B, n_mel, F]) in `dtype`.
    float64: rFFT of the windowed frames.  float32: the twin (windowed DFT basis product, float32 throughout).
    misread: one of MISREADINGS - a deliberately wrong front end for tests/test_mel_restate_cpu.py."""
    assert misread is None or misread in MISREADINGS, misread
    dtype = np.dtype(dtype)
    nbins = n_fft // 2 + 1
    basis = np.asarray(basis)
    assert basis.ndim == 2 and basis.shape[1] == nbins, basis.shape
    win = analysis_window(n_fft, win_length, periodic=misread != "symmetric_window", centred=misread != "uncentred_window")
    fr = frame_matrix(np.asarray(y).astype(dtype), lens, n_fft, hop, misread)
    if dtype == np.float64:
        mag = np.abs(np.fft.rfft(fr * win, axis=-1))
    else:
        w32 = (dft_basis(n_fft, np.ones(n_fft)).astype(np.float32) * win.astype(np.float32)[None, :]).astype(np.float32)
        reim = fr.reshape(-1, n_fft) @ w32.T
        re, im = reim[:, :nbins], reim[:, nbins:]
        mag = np.sqrt(re * re + im * im).reshape(fr.shape[0], fr.shape[1], nbins)
    assert mag.dtype == dtype
    if misread == "energy_kept_bins":
        kept = np.abs(basis).sum(0) != 0
        energy = np.sqrt(((mag * kept) ** 2).sum(-1))
    else:
        energy = np.sqrt((mag * mag).sum(-1))
    mel_lin = np.einsum("nk,bfk->bnf", basis.astype(dtype), mag) if dtype == np.float64 else \
        (mag.reshape(-1, nbins) @ basis.astype(dtype).T).reshape(fr.shape[0], fr.shape[1], -1).transpose(0, 2, 1)
    mel_lin = np.ascontiguousarray(mel_lin)
    mel_log = np.log(np.maximum(mel_lin, dtype.type(clip)))
    return mag, energy.astype(dtype), mel_lin, mel_log


def mel_frontend_scipy32(y, lens, n_fft, hop, win_length, basis, clip=1e-5):
    """float32 through scipy.fft.rfft (which keeps float32): for information only"""
    import scipy.fft
    fr = frame_matrix(np.asarray(y, dtype=np.float32), lens, n_fft, hop) * analysis_window(n_fft, win_length).astype(np.float32)
    mag = np.abs(scipy.fft.rfft(fr, axis=-1)).astype(np.float32)
    energy = np.sqrt((mag * mag).sum(-1))
    mel_lin = np.ascontiguousarray((mag.reshape(-1, mag.shape[-1]) @ np.asarray(basis, dtype=np.float32).T)
                                   .reshape(fr.shape[0], fr.shape[1], -1).transpose(0, 2, 1))
    return mag, energy, mel_lin, np.log(np.maximum(mel_lin, np.float32(clip)))


# ---- the error measures of tests/test_mel_kernels_gpu.py (per frame, never a tensor's global maximum) -----------------------------------------
TINY = 1e-300


def measures(got, ref64, basis, clip=1e-5):
    """got = (mag or None, energy, mel_log) of any evaluation, ref64 = mel_frontend(..., float64) -> dict of worst errors:
      mag     |mag - mag64| / s_f per bin,   energy  |e - e64| / s_f   (s_f = the float64 energy of the frame; frames with s_f = 0 are
              required to be met exactly and count as 0 here, as inf otherwise)
      mel     |max(exp(mel), clip) - max(mel_lin64, clip)| / (||basis[n]||_2 s_f + |ref|), ref = max(mel_lin64, clip)"""
    mag, energy, mel_log = got
    mag64, e64, lin64, _ = ref64
    s = e64.astype(np.float64)
    out = {}

    def ratio(err, scale):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / np.maximum(scale, TINY))
        return float(np.max(r)) if r.size else 0.0

    if mag is not None:
        out["mag"] = ratio(np.abs(np.asarray(mag, dtype=np.float64) - mag64), s[..., None] * np.ones_like(mag64))
    out["energy"] = ratio(np.abs(np.asarray(energy, dtype=np.float64) - e64), s)
    ref = np.maximum(lin64, clip)
    lin = np.maximum(np.exp(np.asarray(mel_log, dtype=np.float64)), clip)
    norm = np.sqrt((np.asarray(basis, dtype=np.float64) ** 2).sum(1))
    out["mel"] = ratio(np.abs(lin - ref), norm[None, :, None] * s[:, None, :] + ref)
    return out


# ---- launch arithmetic of the FFT kernel, restated from its documented constants (a changed constant has to be changed here too) ---------------
NFFT, NBINS, TILE_FILTERS, MS_MAX, KR_CAP, GROUP = 1024, 513, 16, 517, 516, 32


def kmax_of(basis):
    nz = np.nonzero(np.abs(np.asarray(basis)).sum(0) != 0)[0]
    return int(nz.max()) + 1 if len(nz) else 0


def row_stride(kmax):
    """MS: the magnitude tile's row stride for a launch with this kmax (0 = every bin kept)"""
    return (((kmax + 3) & ~3) | 1) if kmax > 0 else MS_MAX


def tile_ranges(basis):
    """per tile of 16 filters: (klo, khi), multiples of 4, (0, 0) for a tile without weight"""
    basis = np.asarray(basis)
    out = []
    for t in range((basis.shape[0] + TILE_FILTERS - 1) // TILE_FILTERS):
        nz = np.nonzero(np.abs(basis[t * TILE_FILTERS:(t + 1) * TILE_FILTERS]).sum(0) != 0)[0]
        out.append((0, 0) if not len(nz) else (int(nz.min()) & ~3, min((int(nz.max()) + 1 + 3) & ~3, KR_CAP)))
    return out


def bank_table(basis, kmax=None):
    """what a launch with this filterbank (and this kmax; None = the filterbank's own) reaches"""
    kmax = kmax_of(basis) if kmax is None else kmax
    ms = row_stride(kmax)
    kr = tile_ranges(basis)
    return dict(n_mel=basis.shape[0], kmax=kmax, MS=ms, keep_low=ms > 256, kr=kr, tiles=len(kr),
                empty_tiles=sum(1 for lo, hi in kr if hi == 0), partial_last_tile=basis.shape[0] % TILE_FILTERS != 0,
                klo0=kr[0][0], group_mods=sorted({(hi - lo) % GROUP for lo, hi in kr if hi > lo}))
