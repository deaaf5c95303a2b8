"""The case table of the waveform-metric tests, shared by tests/test_wavmetrics_restate_cpu.py (which checks that no STOI case has a
frame within 1e-6 dB of its keep threshold) and tests/test_wavmetrics_gpu.py (which therefore compares counts and NaN patterns for
equality on every case).  Signals are float32; no utterance is longer than 3 s at 10 kHz."""
import functools

import numpy as np

SNRS_DB = (30.0, 10.0, 0.0, -10.0)
# F = (len - 256) // 128 + 1: 3839 -> 28 frames, 3840 and 3967 -> 29 (no segment: NaN), 3968 -> 30 (exactly one segment), 4096 -> 31
LENGTHS = (0, 255, 256, 3839, 3840, 3967, 3968, 4096, 6000, 20000, 30000)


def speechlike(n, sr, seed):
    """gliding fundamental + 5 harmonics under a syllable envelope, noise in the unvoiced stretches (as tests/test_loudness_gpu.py)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    f = 150.0 + 60.0 * np.sin(2 * np.pi * (0.7 + 0.3 * rng.random()) * t + rng.random() * 6) + 30.0 * np.sin(2 * np.pi * 2.3 * t)
    ph = 2 * np.pi * np.cumsum(f) / float(sr)
    x = sum(np.sin(k * ph) / k for k in range(1, 7))
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t + rng.random() * 6)
    voiced = np.sin(2 * np.pi * 1.3 * t + rng.random() * 6) > -0.5
    return np.clip(np.where(voiced, 0.3 * x * env, 0.02 * rng.standard_normal(n)), -1, 1).astype(np.float32)


def noise(n, seed, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def mix(x, snr_db, seed):
    """x plus white noise at `snr_db` (power of x over power of the noise), float32"""
    n = np.random.default_rng(seed).standard_normal(len(x))
    if len(x) == 0:
        return n.astype(np.float32)
    px, pn = float(np.mean(x.astype(np.float64) ** 2)), float(np.mean(n ** 2))
    if px == 0.0:
        return (0.01 * n).astype(np.float32)
    return (x.astype(np.float64) + n * np.sqrt(px / pn) * 10.0 ** (-snr_db / 20.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases_10k():
    """[(name, ref, syn)] at 10 kHz"""
    out = []
    for i, n in enumerate(LENGTHS):                                 # white noise: no frame is silent, 3968 samples give one segment
        x = noise(n, 100 + i)
        out.append((f"noise len {n}", x, mix(x, 10.0, 200 + i)))
    sp = speechlike(20000, 10000, 2)
    for snr in SNRS_DB:
        out.append((f"speech-like {snr:+.0f} dB", sp, mix(sp, snr, 300)))
    out.append(("speech-like gain 0.5", sp, (0.5 * sp).astype(np.float32)))
    hole = speechlike(20000, 10000, 3) + noise(20000, 4, 0.01)      # silence in the middle: the compaction crosses tile boundaries
    hole[5000:9000] = 0.0
    hole[12000:14000] *= np.float32(1e-3)
    out.append(("silence in the middle", hole, mix(hole, 10.0, 301)))
    few = noise(8000, 5)
    few[2000:] *= np.float32(1e-4)                                  # 61 frames, fewer than 30 kept
    out.append(("fewer than 30 kept", few, mix(few, 10.0, 302)))
    zero = np.zeros(6000, dtype=np.float32)
    out.append(("all-zero reference", zero, noise(6000, 6)))
    return out


RATE_CASES = ((16000, 30011, 7), (22050, 44100, 8))                 # (rate, samples, seed): 1.9 s and 2 s


@functools.lru_cache(maxsize=None)
def cases_rate(rate):
    """[(name, ref, syn)] at `rate`: speech-like at 10 dB and white noise at 0 dB"""
    _, n, seed = next(c for c in RATE_CASES if c[0] == rate)
    sp, wn = speechlike(n, rate, seed), noise(n - 1234, seed + 10)
    return [(f"speech-like +10 dB @{rate}", sp, mix(sp, 10.0, 400 + seed)), (f"noise 0 dB @{rate}", wn, mix(wn, 0.0, 410 + seed))]
