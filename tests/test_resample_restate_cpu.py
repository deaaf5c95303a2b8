"""CPU: the float64 restatement of the resampler (tests/resample_restate.py) against scipy's polyphase resampler and against the facts
of the `kaiser_best` design, so that the GPU tests stand on a checked reference.

Measured in float64 when the feature was specified (48000 -> 22050, kaiser_best): tones at 100 / 1000 / 8000 Hz reproduced in the
interior to 4e-9 .. 1.1e-8, tones at 12 / 13 / 15 / 20 kHz left below -152 dB.  Asserted with margin for another libm: 1e-6 / -120 dB."""
import math

import numpy as np
import pytest

from tests import resample_restate as R


@pytest.mark.parametrize("a,b", R.RATIOS)
def test_restatement_is_scipy_resample_poly(a, b):
    sig = pytest.importorskip("scipy.signal")
    L, M, half, h = R.design(a, b)
    rng = np.random.default_rng(a + b)
    for n in sorted({1, 2, M - 1, M, M + 1, 1000} - {0}):
        x = rng.standard_normal(n)
        want = sig.resample_poly(x, L, M, window=h / L, padtype="constant")
        got, _, _ = R.resample(x, h, L, M)
        assert got.shape == want.shape == (R.out_len(n, L, M),)
        scale = max(np.abs(want).max(), 1e-300)
        assert np.abs(got - want).max() <= 1e-12 * scale, (a, b, n, np.abs(got - want).max() / scale)


@pytest.mark.parametrize("a,b,n", [(48000, 22050, 7), (22050, 48000, 5), (2, 1, 9), (1, 2, 6), (441, 320, 8)])
def test_gathered_sum_is_the_double_loop(a, b, n):
    L, M, half, h = R.design(a, b, zeros=2)
    x = np.random.default_rng(n).standard_normal(n)
    want = R.resample_direct(x, h, L, M)
    got, mag, terms = R.resample(x, h, L, M)
    assert np.abs(got - want).max() <= 1e-14 * max(1.0, np.abs(want).max())
    assert np.all(mag >= np.abs(got) - 1e-15) and terms.max() <= -(-len(h) // L)
    f32 = R.resample_f32(x, h, L, M)
    assert np.abs(f32 - want).max() <= (terms.max() + 2) * 2.0 ** -24 * mag.max()


def test_reduced_ratios_lengths_and_dc_gain():
    assert R.design(48000, 22050)[:3] == (147, 320, 64 * 320)
    assert R.design(22050, 16000)[:3] == (320, 441, 64 * 441)
    for a, b in R.RATIOS:
        for zeros, beta, rolloff in R.PRESETS.values():
            L, M, half, h = R.design(a, b, zeros, beta, rolloff)
            assert len(h) == 2 * half + 1 and math.gcd(L, M) == 1 and L * a == M * b
            # DC gain.  kaiser_best: 1e-6 as specified.  Any Kaiser design: the ripple 10^(-A / 20) of Kaiser's own formula
            # A = beta / 0.1102 + 8.7 dB (142.7 dB -> 7e-8 for kaiser_best, 86.3 dB -> 4.8e-5 for kaiser_fast)
            ripple = 10.0 ** (-(beta / 0.1102 + 8.7) / 20.0)
            assert abs(h.sum() / L - 1.0) <= (1e-6 if zeros == 64 else ripple), (a, b, zeros, h.sum() / L)
            assert np.abs(h - h[::-1]).max() <= 1e-15 * L                         # linear phase
        for n in (1, 2, M - 1, M, M + 1, 1000):
            assert R.out_len(n, L, M) == math.ceil(n * L / M) == len(R.resample(np.ones(n), h, L, M)[0])


@pytest.fixture(scope="module")
def best_48_to_22():
    return R.design(48000, 22050)


@pytest.mark.parametrize("freq", [100.0, 1000.0, 8000.0])
def test_kaiser_best_passes_tones_up_to_8_khz(best_48_to_22, freq):
    L, M, half, h = best_48_to_22
    n = 16000
    x = np.sin(2 * np.pi * freq * np.arange(n) / 48000.0 + 0.3)
    y, _, _ = R.resample(x, h, L, M)
    ideal = np.sin(2 * np.pi * freq * np.arange(len(y)) / 22050.0 + 0.3)
    mid = slice(len(y) // 4, 3 * len(y) // 4)
    err = np.abs(y[mid] - ideal[mid]).max()
    print(f"{freq} Hz: max |y - ideal| in the middle half {err:.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("freq", [12000.0, 13000.0, 15000.0, 20000.0])
def test_kaiser_best_rejects_tones_from_12_khz(best_48_to_22, freq):
    L, M, half, h = best_48_to_22
    n = 16000
    x = np.sin(2 * np.pi * freq * np.arange(n) / 48000.0 + 0.3)
    y, _, _ = R.resample(x, h, L, M)
    mid = slice(len(y) // 4, 3 * len(y) // 4)
    db = 20 * np.log10(max(np.abs(y[mid]).max(), 1e-300))
    print(f"{freq} Hz: residual {db:.1f} dB")
    assert db <= -120.0


def test_bank_layout_identity():
    for a, b, zeros in [(48000, 22050, 64), (22050, 48000, 16), (2, 1, 4), (1, 2, 4)]:
        L, M, half, h = R.design(a, b, zeros)
        bank = R.bank(h, L)
        h32 = h.astype(np.float32)
        T = -(-len(h) // L)
        assert bank.shape == (L, T)
        for r in range(L):
            for j in range(T):
                i = r + j * L
                assert bank[r, j] == (h32[i] if i < len(h32) else 0.0)
        # y[n] = sum_j bank[r][j] x[k_hi - j] is the same sum
        x = np.random.default_rng(zeros).standard_normal(3 * M + 1)
        want, _, _ = R.resample(x, h32.astype(np.float64), L, M)
        for n in (0, 1, len(want) // 2, len(want) - 1):
            t = n * M + half
            r, k_hi = t % L, t // L
            s = sum(float(bank[r, j]) * x[k_hi - j] for j in range(T) if 0 <= k_hi - j < len(x))
            assert abs(s - want[n]) <= 1e-12 * max(1.0, abs(want[n]))


def test_peak_normalisation_statement():
    x = np.array([0.5, -0.25, 0.1, -0.5], dtype=np.float32)
    v, q, f, ref, wraps = R.peak_normalize(x)
    assert v.tolist() == [32768.0, -16384.0, 6553.60009765625, -32768.0]
    assert q.tolist() == [32767, -16384, 6553, -32768] and wraps.tolist() == [True, False, False, False]
    assert ref.tolist() == [-32768, -16384, 6553, -32768]                    # the reference's wrap of +32768
    assert f.tolist() == [32767 / 32768, -0.5, 6553 / 32768, -1.0]
