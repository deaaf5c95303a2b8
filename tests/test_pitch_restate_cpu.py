"""CPU: the float64 restatements of the pitch-feature kernels (tests/pitch_restate.py) against the live reference's recorded outputs
(tests/golden/g19_pitch_chain.npz), against ground truth (the tracker), against a closed form and the reference's inverse_cwt (the
CWT, whose pycwt parity is unpinned), and the decision margin the GPU tests rely on."""
import math
import os

import numpy as np
import pytest

from tests import pitch_restate as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_pitch_chain.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def tracked_all():
    """(name -> (f0_64, st_64, details_64, f0_32, st_32, details_32, truth), name -> (levels_64, track_pitch keyword arguments)) over
    the ground-truth inputs, the GPU test batches and every case of R.gpu_tracker_cases() ("gpu_case_<name>", run with its parameters)"""
    out, meta = {}, {}
    items = {k: (w[None], None, t, {}) for k, (w, t) in R.ground_truth_inputs().items()}
    items["gpu_batch"] = (R.gpu_tracker_batch(), R.GPU_TRACK_LENS, None, {})
    items["gpu_batch_dense"] = (R.gpu_tracker_batch(), None, None, {})
    items["gpu_silence"] = (R.gpu_silence_batch(), None, None, {})
    for k, c in R.gpu_tracker_cases().items():
        items[f"gpu_case_{k}"] = (c["wav"], c["lens"], c["truth"], c["params"])
    for k, (w, lens, truth, params) in items.items():
        d64, d32, lv = [], [], []
        f64, s64 = R.track_pitch(w, lens, details=d64, levels=lv, **params)
        f32, s32 = R.track_pitch(w, lens, dtype=np.float32, details=d32, **params)
        out[k] = (f64, s64, d64, f32, s32, d32, truth)
        meta[k] = (lv, params)
    return out, meta


@pytest.fixture(scope="module")
def tracked(tracked_all):
    return tracked_all[0]


# ------------------------------------------------------------------------------------------------------------------ chain vs the reference
@pytest.mark.parametrize("k", list(R.FIXTURE_TRACKS))
def test_chain_restatement_matches_reference(gold, k):
    f0 = gold[f"{k}_f0"]
    assert np.array_equal(f0, R.FIXTURE_TRACKS[k])
    uv, c = R.convert_continuous_f0(f0)
    assert np.array_equal(uv, gold[f"{k}_ccf0_uv"]) and uv.dtype == gold[f"{k}_ccf0_uv"].dtype
    np.testing.assert_allclose(c, gold[f"{k}_ccf0"], rtol=0, atol=1e-12)
    uv, lf = R.cont_lf0(f0)
    assert np.array_equal(uv, gold[f"{k}_lf0_uv"])
    g = gold[f"{k}_lf0"]
    assert np.array_equal(np.isfinite(lf), np.isfinite(g))
    np.testing.assert_allclose(lf[np.isfinite(g)], g[np.isfinite(g)], rtol=0, atol=1e-12)
    y, uv2 = R.norm_interp_f0(f0)
    assert np.array_equal(uv2, gold[f"{k}_nif0_uv"])                      # the dataset's polarity: 1 = unvoiced
    assert np.array_equal(uv2, f0 == 0) and np.array_equal(uv2, ~(uv > 0))
    np.testing.assert_allclose(y, gold[f"{k}_nif0"], rtol=0, atol=1e-12)
    ms = gold[f"{k}_mean_std"]
    if np.isfinite(ms).all():
        np.testing.assert_allclose([np.mean(lf), np.std(lf)], ms, rtol=0, atol=1e-12)
    t = R.f0_targets(f0[None], [len(f0)])
    has_w = f"{k}_W" in gold
    assert int(t["valid"][0]) == int(has_w), "valid = 0 exactly for the tracks without two distinct voiced values"
    if has_w:
        W = gold[f"{k}_W"]
        np.testing.assert_allclose(t["cwt_spec"][0], W, rtol=0, atol=1e-12)
        np.testing.assert_allclose([t["f0_mean"][0], t["f0_std"][0]], ms, rtol=0, atol=1e-12)
        nrm, m, s = R.norm_scale(W)
        np.testing.assert_allclose(nrm, gold[f"{k}_norm"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(m, gold[f"{k}_norm_mean"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(s, gold[f"{k}_norm_std"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(R.inverse_cwt(W[None], R.cwt_scales()), gold[f"{k}_icwt"], rtol=0, atol=1e-12)
    else:
        for key in ("uv", "cont_lf0", "cwt_spec", "f0_mean", "f0_std"):
            assert not t[key].any()


def test_by_value_quirk_is_exercised():
    """repeat_first / repeat_last hold the first / last voiced value more than once: the by-value search of :171-172 still lands on the
    first / last voiced index (every frame outside is 0), which is what the kernel uses"""
    for k in ("repeat_first", "repeat_last"):
        f0 = R.FIXTURE_TRACKS[k]
        v = np.where(f0 != 0)[0]
        assert (f0 == f0[v[0]]).sum() > 1 or (f0 == f0[v[-1]]).sum() > 1
        assert np.where(f0 == f0[v[0]])[0][0] == v[0] and np.where(f0 == f0[v[-1]])[0][-1] == v[-1]


# ------------------------------------------------------------------------------------------------------------------ CWT without pycwt
def test_cwt_inverse_reconstructs_contour(gold):
    """(a) Pearson correlation of the reference's inverse_cwt(W) with the normalised contour it came from"""
    worst = 1.0
    for k in R.FIXTURE_TRACKS:
        if f"{k}_W" not in gold:
            continue
        lf = gold[f"{k}_lf0"]
        x = (lf - lf.mean()) / lf.std()
        rec = gold[f"{k}_icwt"][0]
        c = float(np.corrcoef(x, rec)[0, 1])
        c2 = float(np.corrcoef(x, R.inverse_cwt(R.cwt_mexican_hat(x)[None], R.cwt_scales())[0])[0, 1])
        print(f"inverse_cwt correlation {k}: {c:.6f} (restated transform now: {c2:.6f})")
        assert abs(c - c2) < 1e-9
        worst = min(worst, c)
    print(f"inverse_cwt worst correlation {worst:.6f}")
    assert worst >= R.INVERSE_CWT_MIN_CORR - 0.01
    assert R.INVERSE_CWT_MIN_CORR > 0.5


@pytest.mark.parametrize("n,bin_", [(64, 3), (256, 10), (32, 1)])
def test_cwt_closed_form_on_fft_bin(n, bin_):
    """(b) x = cos(w0 t), w0 on an FFT bin, n a power of two: W_j = sqrt(s_j w_1 M) psi(s_j w0) cos(w0 t) - scale, normalisation, sign"""
    t = np.arange(n)
    w1 = 2.0 * np.pi / (n * R.CWT_DT)
    w0 = bin_ * w1
    x = np.cos(w0 * t * R.CWT_DT)
    W = R.cwt_mexican_hat(x)
    for j, s in enumerate(R.cwt_scales()):
        f = s * w0
        expect = math.sqrt(s * w1 * n) * f * f * math.exp(-0.5 * f * f) / math.sqrt(math.gamma(2.5)) * x
        np.testing.assert_allclose(W[:, j], expect, rtol=0, atol=1e-10)
    assert np.abs(W).max() > 0.1
    with pytest.raises(AssertionError):                               # a transform with another normalisation fails this check
        np.testing.assert_allclose(R.cwt_mexican_hat(x, wrong_norm=True), W, rtol=0, atol=1e-10)


def test_cwt_uses_the_utterances_own_power_of_two():
    x = np.random.default_rng(0).standard_normal(37)
    W = R.cwt_mexican_hat(x)
    M = 64
    X = np.fft.fft(x, M)
    w = 2 * np.pi * np.fft.fftfreq(M, R.CWT_DT)
    ref = np.fft.ifft(X * math.sqrt(0.04 * w[1] * M) * R.mexican_hat_ft(0.04 * w))[:37].real
    np.testing.assert_allclose(W[:, 2], ref, atol=1e-12)
    assert R.cwt_mexican_hat(np.ones(1)).shape == (1, 10)


# ------------------------------------------------------------------------------------------------------------------ tracker vs ground truth
def test_tracker_against_ground_truth(tracked):
    worst = 0.0
    for k, (f64, s64, d64, f32, s32, d32, truth) in tracked.items():
        if k.startswith("gpu_"):
            continue
        f = f64[0]
        if truth is None:
            assert not f.any(), f"{k} must be unvoiced"
            continue
        sel = R.full_window_frames(R.GROUND_TRUTH_N)
        assert len(sel) >= 20
        assert (f[sel] > 0).all(), f"{k}: unvoiced frames {sel[f[sel] == 0]}"
        rel = np.abs(f[sel] - truth[sel]) / truth[sel]
        print(f"tracker {k}: worst relative error {rel.max():.3e} over {len(sel)} frames")
        worst = max(worst, float(rel.max()))
    print(f"tracker worst relative error {worst:.6e}")
    assert worst <= 2.0 * R.TRACKER_WORST_REL_ERR
    assert 0 < R.TRACKER_WORST_REL_ERR < 0.02


def test_octave_cost_is_what_rejects_sub_multiples():
    """440 and 700 Hz have 2 tau and 3 tau inside the lag range.  In every full frame of both tones the candidates at 2 tau and 3 tau exist
    with heights within 0.0025 of the fundamental's - less than the 0.01 log2(2) the octave cost puts between them - so the cost, not
    the height, decides.  Measured: without the cost the 700 Hz tone (tau = 31.5, the worst case of the parabola; 2 tau = 63 is an
    integer) falls to 87.5 / 350 Hz in every frame and the 220 Hz tone to 110 Hz in a third of them; the 440 Hz tone (tau = 50.11)
    happens to keep its fundamental by 7e-5 of height, which no tracker may rely on."""
    lo, hi = R.lag_range()
    inputs = R.ground_truth_inputs()
    sel = R.full_window_frames(R.GROUND_TRUTH_N)
    for f in (440.0, 700.0):
        tau = R.SR / f
        assert lo <= tau and 3 * tau <= hi
        w, truth = inputs[f"tone{int(f)}"]
        d = []
        R.track_pitch(w[None], details=d)
        for b, t, lag, h, cost, wi in d:
            if t not in sel:
                continue
            assert abs(lag[wi] - tau) < 0.05, "with the octave cost the fundamental wins"
            for mult in (2, 3):
                near = np.abs(lag - mult * tau) < 0.1
                assert near.sum() == 1, f"{f} Hz frame {t}: no candidate at {mult} tau"
                assert abs(float(h[near][0] - h[wi])) < 0.0025
                assert cost[wi] - cost[near][0] > 0.01 * math.log2(mult) - 0.0025
    for f, frac in ((700.0, 1.0), (220.0, 0.2)):
        w, truth = inputs[f"tone{int(f)}"]
        plain, _ = R.track_pitch(w[None], use_octave_cost=False)
        rel = np.abs(plain[0][sel] - truth[sel]) / truth[sel]
        assert (rel > 0.3).mean() >= frac, f"{f} Hz: a tracker without the octave cost was expected to fall on a sub-multiple"
        assert rel.max() > 2.0 * R.TRACKER_WORST_REL_ERR               # i.e. test_tracker_against_ground_truth fails without the cost


def test_tracker_zero_beyond_length_and_silence(tracked):
    f64, s64 = tracked["gpu_batch"][:2]
    for b, n in enumerate(R.GPU_TRACK_LENS):
        fb = 1 + n // R.HOP
        assert not f64[b, fb:].any() and not s64[b, fb:].any()
        assert (f64[b, :fb] > 0).any()
    f, s = tracked["gpu_silence"][:2]
    assert not f[0].any() and not s[0].any() and np.isfinite(f).all() and (f[1, 2:-2] > 0).all()
    # the second half of utterance 1 is noise: unvoiced there, voiced before
    fb = tracked["gpu_batch"][0][1]
    assert (fb[2:8] > 0).all() and not fb[13:20].any()


# ------------------------------------------------------------------------------------------------------------------ decision margin
def test_decision_margin(tracked_all):
    """delta = 4 x the largest |fp32 - fp64| candidate height; no frame's winner lies within delta of the voicing threshold in use, none
    has a runner-up within delta of the winner's cost, none sits within a relative 1e-3 of the silence threshold in use: fp32 arithmetic
    cannot flip a decision on these inputs, so the GPU tests compare EVERY frame.  An input that fails a margin is replaced, not masked."""
    tracked, meta = tracked_all
    worst_dh, near_thr, near_cost, near_sil = 0.0, np.inf, np.inf, np.inf
    for k, (f64, s64, d64, f32, s32, d32, truth) in tracked.items():
        levels, params = meta[k]
        vthr, sthr = params.get("voicing_threshold", R.VOICING), params.get("silence_threshold", R.SILENCE)
        assert len(d64) == len(d32) == len(levels), k
        k_dh, k_thr, k_cost, k_sil = 0.0, np.inf, np.inf, np.inf
        for (b, t, lag, h, cost, w), (b2, t2, lag2, h2, cost2, w2), (b3, t3, amax, peak) in zip(d64, d32, levels):
            assert (b, t) == (b2, t2) == (b3, t3)
            if len(h) == len(h2):
                k_dh = max(k_dh, float(np.abs(h - h2.astype(np.float64)).max()))
            k_thr = min(k_thr, abs(float(h[w]) - vthr))
            if len(cost) > 1:
                k_cost = min(k_cost, float(cost[w] - np.partition(cost, -2)[-2]))
            if peak > 0:
                k_sil = min(k_sil, abs(amax / (sthr * peak) - 1.0))
        print(f"decision margin {k}: {len(d64)} frames, |fp32 - fp64| height {k_dh:.3e}, voicing {k_thr:.3e}, runner-up {k_cost:.3e}, silence {k_sil:.3e}")
        assert np.array_equal(f64 > 0, f32 > 0), k
        assert k_thr > R.DECISION_DELTA and k_cost > R.DECISION_DELTA and k_sil > 1e-3, k
        worst_dh, near_thr, near_cost, near_sil = max(worst_dh, k_dh), min(near_thr, k_thr), min(near_cost, k_cost), min(near_sil, k_sil)
    delta = 4.0 * worst_dh
    print(f"decision margin: largest |fp32 - fp64| height {worst_dh:.3e} -> delta {delta:.3e}; nearest height to the voicing threshold "
          f"{near_thr:.3e}; smallest winner - runner-up cost gap {near_cost:.3e}; nearest relative distance to the silence threshold {near_sil:.3e}")
    assert R.DECISION_DELTA >= delta, "DECISION_DELTA must cover 4 x the measured fp32 height error"
    assert R.DECISION_DELTA <= 4.0 * delta + 1e-6
    assert near_thr > R.DECISION_DELTA and near_cost > R.DECISION_DELTA and near_sil > 1e-3


# ------------------------------------------------------------------------------------------------------------------ the GPU test's cases
def _case(tracked_all, name):
    f64, s64, d64 = tracked_all[0][f"gpu_case_{name}"][:3]
    return R.gpu_tracker_cases()[name], f64, s64, d64


def test_case_tones_against_ground_truth(tracked_all):
    """every stationary tone of the cases, over the frames whose window lies inside its utterance: voiced, and the worst relative error is
    the recorded TRACKER_TONES_WORST_REL_ERR (the GPU test asserts 2 x it against the true frequency)"""
    worst, seen = 0.0, 0
    for name, c in R.gpu_tracker_cases().items():
        f64 = tracked_all[0][f"gpu_case_{name}"][0]
        for b, hz in enumerate(c["truth"]):
            if hz is None:
                continue
            sel = R.full_window_frames(R.case_length(c, b), c["params"].get("hop", R.HOP))
            assert len(sel) >= 8 and (f64[b, sel] > 0).all(), (name, b)
            rel = float((np.abs(f64[b, sel] - hz) / hz).max())
            print(f"tracker case {name}[{b}] {hz:g} Hz: worst relative error {rel:.3e} over {len(sel)} frames")
            worst, seen = max(worst, rel), seen + 1
    print(f"tracker cases: worst relative error {worst:.6e} over {seen} tones")
    assert seen == 15
    assert 0.9 * R.TRACKER_TONES_WORST_REL_ERR <= worst <= R.TRACKER_TONES_WORST_REL_ERR < 0.02


def test_cases_reach_the_lag_range_they_claim(tracked_all):
    """what the inputs are for: winners in every register m = lag // 64 of pitch_track_kernel from 0 to 7, a winner next to lag_lo, the
    sub-multiples of 440 and 700 Hz rejected by the cost and not the height on the float32 batch as well"""
    seen = set()
    for name in R.gpu_tracker_cases():
        c, f64, s64, d64 = _case(tracked_all, name)
        sr, p = c["params"].get("sr", R.SR), {k: v for k, v in c["params"].items() if k in ("sr", "f0_min", "f0_max")}
        lo, hi = R.lag_range(**p)
        for b, t, lag, h, cost, w in d64:
            if f64[b, t] > 0:
                seen.add(int(round(lag[w])) // 64)
        if name == "edges":
            by_row = {b: [lag[w] for bb, t, lag, h, cost, w in d64 if bb == b and f64[b, t] > 0] for b in range(4)}
            assert min(by_row[0]) > 256 and min(by_row[1]) > 256            # 81, 84 Hz: m = 4
            assert lo == 29 and all(29.5 < v < 30.5 for v in by_row[2])    # 740 Hz: integer lag 30, its neighbour lag_lo itself
        if name == "f0min50":
            assert hi == 441 and all((384 if b == 0 else 320) <= lag[w] for b, t, lag, h, cost, w in d64 if f64[b, t] > 0)
    assert seen == set(range(8)), seen
    c, f64, s64, d64 = _case(tracked_all, "ground_truth")
    plain, _ = R.track_pitch(c["wav"][4:5], use_octave_cost=False)
    sel = R.full_window_frames(R.GROUND_TRUTH_N)
    assert (np.abs(plain[0, sel] - 700.0) / 700.0 > 0.3).all() and (np.abs(f64[4, sel] - 700.0) / 700.0 < 1e-3).all()


def test_ragged_case_lengths(tracked_all):
    for name in ("ragged", "ragged_sr16k", "sr16k", "sr48k"):
        c, f64, s64, d64 = _case(tracked_all, name)
        hop = c["params"].get("hop", R.HOP)
        assert f64.shape == (len(c["wav"]), 1 + R.GROUND_TRUTH_N // hop)
        for b in range(len(c["wav"])):
            fb = 1 + R.case_length(c, b) // hop
            assert not f64[b, fb:].any() and not s64[b, fb:].any()
    c, f64, s64, d64 = _case(tracked_all, "ragged")
    assert [R.case_length(c, b) for b in range(5)] == [6000, 100, 6144, 0, 3333]
    assert not any(n % R.HOP == 0 for n in R.RAGGED_LENS) and (5 * f64.shape[1]) % 16 and f64.shape[1] % 4
    assert (f64[0, :24] > 0).all() and (f64[2] > 0).all() and (f64[4, :14] > 0).all()
    assert s64[1, 0] > 0 and not f64[1].any() and not s64[3].any() and not f64[3].any()
    assert np.abs(c["wav"][3]).max() > 0.5 and np.abs(c["wav"][1, 100:]).max() > 0.5, "garbage beyond the lengths"


def test_threshold_cases(tracked_all):
    """silence_threshold: the 2 % tail of utterance 0 is unvoiced at 0.03 and voiced at 0.01; utterance 1, whose peak is 2.4 % of utterance
    0's, is voiced at both - it would be silent at 0.03 under a peak taken over the batch.  voicing_threshold: every full frame of the
    tone in noise has its winner between 0.4 and 0.6.  Neither threshold touches the strength."""
    c, f_def, s_def, _ = _case(tracked_all, "silence_default")
    _, f_low, s_low, _ = _case(tracked_all, "silence_low")
    assert np.array_equal(s_def, s_low)
    quiet = [t for t in range(f_def.shape[1]) if t * R.HOP - R.FRAME // 2 >= R.SILENCE_STEP]
    loud = [t for t in R.full_window_frames(R.SILENCE_STEP)]
    assert len(quiet) >= 10 and len(loud) >= 8
    assert not f_def[0, quiet].any() and (f_low[0, quiet] > 0).all() and (s_def[0, quiet] > 0.65).all()
    assert (f_def[0, loud] > 0).all() and (f_low[0, loud] > 0).all()
    assert (f_def[1] > 0).all() and (f_low[1] > 0).all()
    peaks = np.abs(c["wav"]).max(1)
    assert R.SILENCE_LOW * peaks[0] * 1.1 < peaks[1] < R.SILENCE * peaks[0] * 0.9
    c, f_def, s_def, _ = _case(tracked_all, "voicing_default")
    _, f_low, s_low, _ = _case(tracked_all, "voicing_low")
    assert np.array_equal(s_def, s_low)
    sel = R.full_window_frames(R.GROUND_TRUTH_N)
    assert (s_def[0, sel] > R.VOICING_LOW + 0.02).all() and (s_def[0, sel] < R.VOICING - 0.005).all()
    assert not f_def.any() and (f_low[0, sel] > 0).all()


def test_chain_edge_inputs():
    """the target-chain inputs of the GPU test: every length of the size-edge batches gives a valid utterance in float64 and float32,
    except n = 2 - at M = 2 pycwt's w_1 = 2 pi fftfreq(2, dt)[1] is negative, sqrt(s_j w_1 M) is NaN and the non-finite rule drops the
    utterance although its contour has two distinct values; the long runs have the lengths they claim"""
    with np.errstate(invalid="ignore"):
        assert np.isnan(R.cwt_mexican_hat(np.array([-1.0, 1.0]))).all() and np.isfinite(R.cwt_mexican_hat(np.array([-1.0, 0.0, 1.0]))).all()
    for f0, frames in R.gpu_chain_edge_batches():
        assert f0.dtype == np.float32 and f0.shape == (len(frames), max(frames))
        for dt in (np.float64, np.float32):
            assert R.f0_targets(f0, frames, dtype=dt)["valid"].tolist() == [int(n != 2) for n in frames]
        for b, n in enumerate(frames):
            assert (f0[b, n:] > 0).all() or n == f0.shape[1], "garbage beyond the length"
    assert sorted(n for fr in R.CHAIN_EDGE_FRAMES for n in fr) == [2, 3, 255, 256, 257, 512, 513, 2048, 2049]
    f0, frames = R.gpu_chain_long_runs()
    n = R.CHAIN_LONG_N
    assert frames == (n,) * 5 and f0.shape == (5, n)
    assert not f0[0, :700].any() and f0[0, 700] > 0
    assert f0[1, 999] > 0 and not f0[1, 1000:2500].any() and f0[1, 2500] > 0
    assert f0[2, n - 601] > 0 and not f0[2, n - 600:].any()
    assert np.flatnonzero(f0[3]).tolist() == [0, n - 1] and np.flatnonzero(f0[4]).tolist() == [2000]
    for dt in (np.float64, np.float32):
        assert R.f0_targets(f0, frames, dtype=dt)["valid"].tolist() == [1, 1, 1, 1, 0]


def test_float32_twin_is_float32():
    w = R.gpu_tracker_batch()[:1, :2048]
    f, s = R.track_pitch(w, dtype=np.float32)
    assert f.dtype == np.float32 and s.dtype == np.float32
    t = R.f0_targets(R.gpu_chain_batch(), R.CHAIN_FRAMES, dtype=np.float32)
    assert t["cwt_spec"].dtype == np.float32 and t["cont_lf0"].dtype == np.float32
    assert np.array_equal(t["valid"], [1, 1, 1, 0])
    t64 = R.f0_targets(R.gpu_chain_batch(), R.CHAIN_FRAMES)
    assert np.array_equal(t64["valid"], [1, 1, 1, 0])
    assert 0 < np.abs(t["cwt_spec"] - t64["cwt_spec"]).max() < 1e-4
    f0, frames = R.gpu_chain_invalid_batch()
    assert np.array_equal(R.f0_targets(f0, frames)["valid"], [0, 0, 1])
