"""The filterbanks, signals and expected launch table of tests/test_mel_restate_cpu.py and tests/test_mel_kernels_gpu.py (host numpy only).
The Slaney banks come from ctts_amd.audio.slaney_mel_basis (pinned by tests/test_mel_basis_cpu.py); the synthetic ones are built here."""
import numpy as np

from ctts_amd.audio import slaney_mel_basis

SR, NFFT, NBINS = 22050, 1024, 513

# (n_mel, fmin, fmax) at n_fft 1024, sr 22050
REAL_BANKS = [(80, 0, 8000), (80, 0, None), (40, 0, 4000), (17, 300, 5400), (96, 0, 1500), (96, 0, None), (33, 0, 5480),
              (80, 2000, 11025), (1, 0, 8000), (16, 0, 8000)]
SYNTHETIC_BANKS = ["dense", "empty_tile", "mod0", "mod4", "mod28"]


def bank_name(spec):
    return spec if isinstance(spec, str) else f"{spec[0]}mel_{spec[1]}_{spec[2]}"


def banded(ranges, seed):
    """80 filters whose tile t (16 filters) carries random weight in (0.01, 1] on every bin of ranges[t] = [lo, hi) and none elsewhere"""
    rng = np.random.RandomState(seed)
    w = np.zeros((80, NBINS), dtype=np.float32)
    for t, (lo, hi) in enumerate(ranges):
        w[16 * t:16 * t + 16, lo:hi] = rng.uniform(0.01, 1.0, size=(16, hi - lo)).astype(np.float32)
    return w


def filterbank(spec):
    """spec: an entry of REAL_BANKS or SYNTHETIC_BANKS -> float32 [n_mel, 513]"""
    if not isinstance(spec, str):
        return slaney_mel_basis(SR, NFFT, spec[0], spec[1], spec[2])
    if spec == "dense":            # every bin, bin 512 included, carries weight in every filter: kmax 513, MS 517, every tile (0, 516)
        return np.random.RandomState(11).uniform(0.0, 0.02, size=(80, NBINS)).astype(np.float32) + np.float32(1e-4)
    if spec == "empty_tile":       # the 80 / 0-8000 bank with the filters of tile 1 removed
        w = slaney_mel_basis(SR, NFFT, 80, 0, 8000)
        w[16:32] = 0
        return w
    # tiles whose bin range leaves (khi - klo) % 32 = 0, 4, 28: whole groups only / a last group of one step / one of seven steps, no whole one
    if spec == "mod0":
        return banded([(8, 72), (40, 72), (100, 196), (8, 40), (64, 96)], 12)
    if spec == "mod4":
        return banded([(8, 44), (41, 75), (100, 136), (9, 12), (64, 164)], 13)
    if spec == "mod28":
        return banded([(8, 36), (40, 68), (101, 127), (8, 100), (64, 92)], 14)
    raise KeyError(spec)


# what the issue states for the real banks, (kmax, MS); checked against tests/mel_restate.bank_table
STATED = {(40, 0, 4000): (186, 189), (17, 300, 5400): (None, 253), (96, 0, 1500): (None, 73), (33, 0, 5480): (255, 257),
          (80, 0, None): (512, 513), (96, 0, None): (512, 513), (80, 0, 8000): (372, 373)}


# ---- signals at [B, N] (float32, inside [-1, 1]) ------------------------------------------------------------------------------------------
SIGNALS = ["noise", "tone_centred", "tone_off_centre", "tone_bin256", "tone_bin512", "dc", "impulse_first", "impulse_last",
           "impulse_frame_centre", "loud_then_zeros", "glide_beside_noise"]


def signal(name, B, N, hop=256, seed=0):
    rng = np.random.RandomState(1000 + seed)
    n = np.arange(N, dtype=np.float64)
    y = np.zeros((B, N), dtype=np.float64)
    if name == "noise":
        y = rng.uniform(-0.9, 0.9, size=(B, N))
    elif name == "tone_centred":
        for b in range(B):
            y[b] = 0.7 * np.cos(2 * np.pi * (40 + 100 * b) * n / NFFT + 0.3)
    elif name == "tone_off_centre":
        for b in range(B):
            y[b] = 0.7 * np.cos(2 * np.pi * (57.37 + 131.2 * b) * n / NFFT + 1.1)
    elif name == "tone_bin256":
        y[:] = 0.8 * np.cos(2 * np.pi * 256 * n / NFFT + 0.2)
    elif name == "tone_bin512":
        y[:] = 0.8 * np.cos(np.pi * n)
    elif name == "dc":
        y[:] = 0.5
    elif name == "impulse_first":
        y[:, 0] = 1.0
    elif name == "impulse_last":
        y[:, N - 1] = 1.0
    elif name == "impulse_frame_centre":
        y[:, 5 * hop] = 1.0
        y[-1, 6 * hop] = -1.0
    elif name == "loud_then_zeros":      # hop 256: frames from 7 on hold exact zeros only (frame 7 starts at sample 7 * 256 - 512 = 1280)
        y[:, :5 * hop] = rng.uniform(-0.9, 0.9, size=(B, 5 * hop))
    elif name == "glide_beside_noise":   # 60 dB between neighbouring frames: five harmonics at 0.3 in the first half, 1e-3 noise after it
        half = (N // (2 * hop)) * hop
        f0 = 110.0 + 90.0 * n[:half] / half
        ph = 2 * np.pi * np.cumsum(f0) / SR
        for b in range(B):
            y[b, :half] = 0.3 / 5 * sum(np.cos((h + 1) * ph * (1 + 0.5 * b)) for h in range(5))
            y[b, half:] = 1e-3 * rng.uniform(-1, 1, size=N - half)
        y = np.clip(y, -1, 1)
    else:
        raise KeyError(name)
    return y.astype(np.float32)
