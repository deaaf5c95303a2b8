"""CPU: pins tests/wavmetrics_restate.py, the float64 statement of the waveform metrics the kernels of csrc/wavmetrics.hip are tested
against, and the fairness condition on the shared case table (tests/wavmetrics_inputs.py)."""
import math

import numpy as np
import pytest

from tests import wavmetrics_inputs as I
from tests import wavmetrics_restate as R

EDGES = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138),
         (138, 174), (174, 219)]


def test_band_edge_table():
    assert R.band_edges() == EDGES
    w = R.window()
    assert len(w) == 256 and w[0] > 0 and np.allclose(w, w[::-1]) and abs(w[127] - math.sin(math.pi * 128 / 257) ** 2) < 1e-15


def test_stoi_of_a_signal_with_itself_and_snr_ordering():
    x = I.speechlike(20000, 10000, 2)
    same = R.stoi(x, x)
    assert abs(same["stoi"] - 1.0) <= 1e-12 and abs(same["estoi"] - 1.0) <= 1e-12
    got = [R.stoi(x, I.mix(x, snr, 300)) for snr in I.SNRS_DB]
    for key in ("stoi", "estoi"):
        v = [g[key] for g in got]
        print(key, ["%.3f" % a for a in v])
        assert 1.0 > v[0] > v[1] > v[2] > v[3] > 0.0, (key, v)


def test_si_sdr_equals_the_constructed_ratio_and_ignores_gain():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(5000)
    x -= x.mean()
    for s in (30.0, 10.0, 0.0, -10.0):
        n = rng.standard_normal(5000)
        n -= n.mean()
        n -= np.dot(n, x) / np.dot(x, x) * x                       # orthogonal to x
        n *= math.sqrt(np.dot(x, x) / np.dot(n, n)) * 10.0 ** (-s / 20.0)
        y = x + n
        assert abs(R.si_sdr(x, y) - s) <= 1e-9
        for g in (0.25, 3.7):
            assert abs(R.si_sdr(x, g * y) - s) <= 1e-9
    assert math.isinf(R.si_sdr(x.astype(np.float32), 0.5 * x.astype(np.float32)))
    assert math.isnan(R.si_sdr(np.zeros(0), np.zeros(0))) and math.isnan(R.si_sdr(np.zeros(10), np.ones(10)))
    assert math.isnan(R.si_sdr(np.full(10, 0.25), np.arange(10.0)))                 # a constant reference: <x,x> = 0 once the mean is removed


def test_mr_stft_of_a_gain_only_copy():
    x = I.noise(9000, 1, 0.3).astype(np.float64)
    for g in (0.5, 1.7):
        d = R.mr_stft_distance(x, g * x)
        for r, (n_fft, hop, win) in enumerate(R.MR_DEFAULT):
            mag = np.abs(np.fft.rfft(x[:win] * R.mr_window(win), n=n_fft))
            assert min(mag.min(), g * mag.min()) ** 2 > R.MR_CLAMP                  # the clamp is inactive (checked on the first frame)
            assert abs(d["sc"][r] - abs(1 - g)) <= 1e-12
            assert abs(d["log_mag"][r] - abs(math.log(g))) <= 1e-12
            assert abs(d["lsd_db"][r] - abs(20 * math.log10(g))) <= 1e-11
            assert d["frames"][r] == (9000 - win) // hop + 1


def test_nan_and_count_rules():
    x = I.noise(4096, 1)
    y = I.mix(x, 10.0, 2)
    # F = (len - 256) // 128 + 1: the 30th frame ends at sample 29 * 128 + 256 = 3968
    for n, frames, segments in ((0, 0, 0), (255, 0, 0), (256, 1, 0), (3839, 28, 0), (3840, 29, 0), (3967, 29, 0), (3968, 30, 1), (4095, 30, 1),
                                (4096, 31, 2)):
        v = R.stoi(x[:n], y[:n])
        assert (v["frames"], v["segments"]) == (frames, segments) and v["kept"] == frames       # white noise: no frame is silent
        assert math.isnan(v["stoi"]) == math.isnan(v["estoi"]) == (segments == 0)
    zero = R.stoi(np.zeros(6000, dtype=np.float32), I.noise(6000, 6))
    assert zero["frames"] == 45 and zero["kept"] == 45 and zero["segments"] == 0 and math.isnan(zero["stoi"])
    name, few, fy = next(c for c in I.cases_10k() if c[0] == "fewer than 30 kept")
    v = R.stoi(few, fy)
    assert v["frames"] == 61 and 0 < v["kept"] < 30 and v["segments"] == 0 and math.isnan(v["estoi"])
    name, hole, hy = next(c for c in I.cases_10k() if c[0] == "silence in the middle")
    v = R.stoi(hole, hy)
    assert v["frames"] == 155 and 30 <= v["kept"] < 155 - 40 and v["segments"] == v["kept"] - 29
    for n_fft, hop, win in R.MR_DEFAULT:
        assert R.stft_distance(x[:win - 1], y[:win - 1], n_fft, hop, win)[3] == 0
        assert math.isnan(R.stft_distance(x[:win - 1], y[:win - 1], n_fft, hop, win)[0])
        assert R.stft_distance(x[:win], y[:win], n_fft, hop, win)[3] == 1
    with pytest.raises(AssertionError):
        R.stft_distance(x, y, 256, 64, 256)
    with pytest.raises(AssertionError):
        R.stft_distance(x, y, 512, 64, 513)


def test_float32_evaluation_is_close_but_not_equal():
    name, x, y = next(c for c in I.cases_10k() if c[0] == "speech-like +10 dB")
    a, b = R.stoi(x, y), R.stoi(x, y, dtype=np.float32)
    assert (a["frames"], a["kept"], a["segments"]) == (b["frames"], b["kept"], b["segments"])
    assert 0 < abs(a["stoi"] - b["stoi"]) < 1e-4 and 0 < abs(a["estoi"] - b["estoi"]) < 1e-4
    assert 0 < abs(R.si_sdr(x, y) - R.si_sdr(x, y, dtype=np.float32)) < 1e-3
    m64, m32 = R.mr_stft_distance(x, y), R.mr_stft_distance(x, y, dtype=np.float32)
    for key in ("sc", "log_mag", "lsd_db"):
        assert np.all(np.abs(m64[key] - m32[key]) < 1e-3) and np.any(m64[key] != m32[key])


def test_no_frame_of_the_case_table_sits_on_its_keep_threshold():
    """what makes it fair for the GPU test to demand equal counts on every case: the nearest frame energy is 1e-6 dB from max - 40,
    seven orders of magnitude more than two double evaluations of 20 log10(||w x|| + eps) can differ by"""
    for name, x, _ in I.cases_10k():
        margin = R.threshold_margin_db(x)
        assert margin > 1e-6, (name, margin)
