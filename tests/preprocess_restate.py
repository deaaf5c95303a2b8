"""Float64 numpy restatements of the three dataset-preparation steps (include/ctts.h "Dataset preparation on the device"): the yardstick of
tests/test_preprocess_gpu.py, itself pinned against the live reference by tests/test_preprocess_restate_cpu.py (the prior, the outlier
filter and the scaler; librosa is not installed, so the trim restates librosa 0.7.2's published `effects.trim` and pins nothing about it).
"""
import math

import numpy as np

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def frame_power(x, frame_length=1024, hop=256):
    """mse_f of `effects.trim`: reflect-pad by frame_length / 2, frames f = 0 .. len // hop, mean of squares over frame_length samples"""
    x = np.asarray(x, dtype=np.float64)
    if len(x) <= frame_length // 2:
        raise ValueError("reflection needs more than frame_length / 2 samples")
    xp = np.pad(x, frame_length // 2, mode="reflect")
    nf = 1 + len(x) // hop
    return np.array([np.mean(xp[f * hop:f * hop + frame_length] ** 2) for f in range(nf)])


def frame_db(x, frame_length=1024, hop=256):
    """10 log10(max(1e-10, mse_f)) - 10 log10(max(1e-10, max_f mse_f)): power_to_db(ref=np.max, top_db=None)"""
    mse = frame_power(x, frame_length, hop)
    return 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))


def trim_silence(x, top_db, frame_length=1024, hop=256):
    """-> (start, end) in samples; (0, 0) without a non-silent frame"""
    nz = np.flatnonzero(frame_db(x, frame_length, hop) > -top_db)
    if nz.size == 0:
        return 0, 0
    return int(hop * nz[0]), int(min(len(x), hop * (nz[-1] + 1)))


def attention_prior(n_phones, n_frames, scaling_factor=1.0):
    """[n_phones, n_frames] float64: out[s, t] = BetaBinom.pmf(t; n = n_frames, a = sf (s + 1), b = sf (n_phones - s)), closed form"""
    P, n, sf = int(n_phones), int(n_frames), float(scaling_factor)
    s = np.arange(P, dtype=np.float64)[:, None]
    k = np.arange(n, dtype=np.float64)[None, :]
    a, b = sf * (s + 1.0), sf * (P - s)
    logp = (_lgamma(n + 1.0) - _lgamma(k + 1.0) - _lgamma(n - k + 1.0) + _lgamma(k + a) + _lgamma(n - k + b) - _lgamma(n + a + b)
            - _lgamma(a) - _lgamma(b) + _lgamma(a + b))
    return np.exp(logp)


def attention_prior_batch(src_lens, mel_lens, Ts, Tm, scaling_factor=1.0):
    """the zero-padded [B, Ts, Tm] batch of `pad_3D` / `data.reprocess`"""
    out = np.zeros((len(src_lens), Ts, Tm), dtype=np.float64)
    for i, (p, m) in enumerate(zip(src_lens, mel_lens)):
        out[i, :p, :m] = attention_prior(p, m, scaling_factor)
    return out


def outlier_bounds(v):
    """(lower, upper) of `remove_outlier`: numpy's default (linear) percentiles, position q (n - 1), in float64"""
    srt = np.sort(np.asarray(v, dtype=np.float64))
    n = len(srt)

    def pct(q):
        pos = q * (n - 1)
        lo = int(math.floor(pos))
        hi = min(lo + 1, n - 1)
        return srt[lo] + (srt[hi] - srt[lo]) * (pos - lo)
    p25, p75 = pct(0.25), pct(0.75)
    return p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)


def outlier_keep(v):
    lower, upper = outlier_bounds(v)
    v = np.asarray(v, dtype=np.float64)
    return (v > lower) & (v < upper)


def bound_margin(v):
    """smallest relative distance of a value to either bound (inf when there is none): the tests require it to stay above 1e-5.
    With p25 == p75 (n = 1, a constant array, both quartiles inside one run of equal values) both bounds ARE that value, bit for bit in
    any precision (x0 + (x1 - x0) * frac with x1 == x0), so values equal to it are rejected exactly and do not count as near."""
    lower, upper = outlier_bounds(v)
    v = np.asarray(v, dtype=np.float64)
    if lower == upper:
        v = v[v != lower]
    if v.size == 0:
        return np.inf
    scale = max(abs(lower), abs(upper), np.abs(v).max(), 1e-300)
    return min(np.abs(v - lower).min(), np.abs(v - upper).min()) / scale


def moments(v):
    """(count, sum, M2) of the kept values, M2 about their own mean"""
    kept = np.asarray(v, dtype=np.float64)[outlier_keep(v)]
    if kept.size == 0:
        return 0, 0.0, 0.0
    return int(kept.size), float(kept.sum()), float(((kept - kept.mean()) ** 2).sum())


def dataset_mean_std(arrays):
    """mean / population std of the concatenated kept values = what StandardScaler.partial_fit converges to"""
    kept = [np.asarray(v, dtype=np.float64)[outlier_keep(v)] for v in arrays]
    allv = np.concatenate([k for k in kept if k.size])
    return float(allv.mean()), float(allv.std())


def assert_prior_close(got, want, what):
    """THE bar of the prior, on the CPU and on the GPU: relative <= 1e-6 wherever `want` >= 1e-30, absolute <= 1e-37 below"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    big = want >= 1e-30
    rel = np.abs(got[big] - want[big]) / want[big]
    print(f"{what}: {int(big.sum())} entries >= 1e-30, max rel {rel.max() if rel.size else 0.0:.3e}; "
          f"{int((~big).sum())} below, max abs {np.abs(got[~big] - want[~big]).max() if (~big).any() else 0.0:.3e}")
    assert rel.size == 0 or rel.max() <= 1e-6, (what, rel.max())
    assert (~big).sum() == 0 or np.abs(got[~big] - want[~big]).max() <= 1e-37, what


# ---- fixtures shared by the golden generator and the tests -----------------------------------------------------------------------
PRIOR_CASES = [(1, 1, 1.0), (7, 3, 1.0), (3, 7, 1.0), (40, 9, 0.5), (440, 55, 1.0)]      # (P, M, sf) as the reference is CALLED: P = frames
PRIOR_BIG = (1000, 128, 1.0)
PRIOR_BIG_ROWS = [0, 1, 63, 126, 127]


def outlier_fixtures():
    """name -> float32 array: lengths 1, 2, 3, 4, 5, 101, 870 (seeded, with a few far outliers), one constant array and one whose
    quartile positions fall on runs of equal values"""
    rng = np.random.default_rng(20)
    out = {}
    for n in (1, 2, 3, 4, 5, 101, 870):
        v = rng.normal(37.0, 9.0, n)
        if n >= 5:
            v[rng.choice(n, max(1, n // 40), replace=False)] += rng.choice([-1.0, 1.0], max(1, n // 40)) * rng.uniform(60.0, 200.0, max(1, n // 40))
        out[f"n{n}"] = v.astype(np.float32)
    out["const"] = np.full(17, 3.25, dtype=np.float32)
    out["ties"] = np.array([1.0] * 6 + [2.0] * 7 + [3.0] * 6 + [2.5, 9.0, -7.0, 2.0], dtype=np.float32)      # sorted: 25 % and 75 % sit inside runs
    return out
