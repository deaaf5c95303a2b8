"""CPU: pins tests/loudness_restate.py, the float64 definition the loudness kernels are tested against, to the standard itself - the
BS.1770-4 filter table at 48 kHz, the conformance tones of EBU Tech 3341, the two gates and the block bookkeeping - and the host-side
design of ctts_amd.loudness (biquads, state-transition matrix, block tables) to the restatement.  No GPU, no pyloudnorm.

Measured here: the RBJ design of the restatement differs from the standard's 48 kHz table by at most 0.04312 dB in magnitude between
20 Hz and 20 kHz, nearly all of it a constant: the table's high pass has b = [1, -2, 1] where the design has b0 = (1 + cos w0) / 2 / a0
= 0.99504 (20 log10 of that is -0.0432 dB).  The test pins the difference at twice the measured value."""
import math
import os
import sys

import numpy as np
import pytest
from scipy.signal import freqz, lfilter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_restate as R  # noqa: E402

TABLE_48K = (([1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -1.69065929318241, 0.73248077421585]),
             ([1.0, -2.0, 1.0], [1.0, -1.99004745483398, 0.99007225036621]))
DESIGN_VS_TABLE_DB = 0.04312          # measured (module docstring); > 0.1 dB would mean mis-transcribed formulas


def _sine(freq, amp, rate, seconds):
    return amp * np.sin(2 * np.pi * freq * np.arange(int(seconds * rate)) / rate)


def test_design_against_the_standards_table():
    f = np.geomspace(20.0, 20000.0, 4096)
    tab = np.ones_like(f, dtype=np.complex128)
    des = np.ones_like(f, dtype=np.complex128)
    for (tb, ta), (b, a) in zip(TABLE_48K, R.kweighting(48000)):
        tab = tab * freqz(tb, ta, worN=f, fs=48000)[1]
        des = des * freqz(b, a, worN=f, fs=48000)[1]
        assert a[0] == 1.0
    diff = float(np.max(np.abs(20 * np.log10(np.abs(des)) - 20 * np.log10(np.abs(tab)))))
    print(f"K-weighting design vs BS.1770-4 table at 48 kHz: {diff:.5f} dB")
    assert diff < 0.1
    assert diff <= 2 * DESIGN_VS_TABLE_DB


@pytest.mark.parametrize("rate", [48000, 22050, 16000])
@pytest.mark.parametrize("amp,expect", [(1.0, -3.01), (10 ** (-23 / 20), -26.01)])
def test_conformance_tone(rate, amp, expect):
    L, valid = R.integrated_loudness(_sine(997.0, amp, rate, 5.0), rate)
    print(f"{rate} Hz, amplitude {amp:.4f}: {L:.4f} LUFS")
    assert valid == 1 and abs(L - expect) <= 0.1


def test_relative_gate_removes_the_quiet_stretch():
    rate = 22050
    loud = _sine(997.0, 0.5, rate, 4.0)
    both = np.concatenate([loud, _sine(997.0, 0.5 * 10 ** (-25 / 20), rate, 4.0)])
    L1, _ = R.integrated_loudness(loud, rate)
    L2, _ = R.integrated_loudness(both, rate)
    # the 37 blocks inside the loud stretch count whole, the three that straddle the step pass the gate with 3/4, 1/2 and 1/4 of its
    # energy, and every block of the quiet stretch (25 dB down, the gate sits 10 LU under the mean) is removed
    assert abs(L2 - (L1 + 10 * math.log10(38.5 / 40))) < 0.01
    ungated = -0.691 + 10 * math.log10(np.mean(R.block_energies(both, rate)))
    assert L1 - ungated > 2.5                        # without the gate the quiet half would pull the mean down by about 3 dB


def test_absolute_gate_ignores_digital_silence():
    rate = 16000
    x = _sine(440.0, 0.1, rate, 3.0)
    L1, _ = R.integrated_loudness(x, rate)
    L2, _ = R.integrated_loudness(np.concatenate([x, np.zeros(5 * rate)]), rate)
    L3, _ = R.integrated_loudness(np.concatenate([x, np.zeros(50 * rate)]), rate)
    assert abs(L3 - L2) < 1e-9                       # how much silence follows does not matter: its blocks lie under -70 LUFS
    # what remains is the three blocks that straddle the end of the tone (3/4, 1/2, 1/4 full) beside the 27 whole ones
    assert abs(L2 - (L1 + 10 * math.log10(28.5 / 30))) < 0.01
    l = R.momentary(np.concatenate([x, np.zeros(5 * rate)]), rate)
    assert np.all(l[31:] < R.ABSOLUTE_GATE) and np.all(l[:30] > -40.0)


def test_all_silence():
    L, valid = R.integrated_loudness(np.zeros(22050), 22050)
    assert L == -math.inf and valid == 0
    out, L, gain, valid = R.normalize(np.zeros(22050), 22050)
    assert gain == 1.0 and valid == 0 and not out.any()


@pytest.mark.parametrize("rate", [48000, 22050, 11025])
def test_block_bookkeeping(rate):
    rng = np.random.default_rng(rate)
    block = 0.4 * rate
    for seconds, want in ((0.4, 1), (0.449, 1), (0.451, 2)):
        n = int(math.ceil(seconds * rate))
        x = rng.standard_normal(n)
        z = R.block_energies(x, rate)
        assert len(z) == want == R.n_blocks(n, rate)
        y = lfilter(*R.kweighting(rate)[1], lfilter(*R.kweighting(rate)[0], x))
        assert z[0] == pytest.approx(np.sum(y[:int(block)] ** 2) / block, rel=1e-12)
        if want == 2:
            lo = int(0.4 * 0.25 * rate)
            assert R.block_bounds(1, rate) == (lo, int(0.4 * 1.25 * rate)) and R.block_bounds(1, rate)[1] > n
            assert z[1] == pytest.approx(np.sum(y[lo:] ** 2) / block, rel=1e-12)      # cut at n, divided by the whole block
    with pytest.raises(ValueError):
        R.block_energies(np.zeros(int(block) - 1), rate)


def test_hop_is_not_a_whole_number_of_samples_at_11025():
    lo = [R.block_bounds(j, 11025)[0] for j in range(6)]
    assert lo == [0, 1102, 2205, 3307, 4410, 5512]
    assert len(R.momentary(np.ones(11025), 11025)) == 7
    assert len(R.short_term(np.ones(4 * 11025), 11025)) == 11


def test_normalisation_reaches_the_target():
    rate = 22050
    x = 0.05 * np.random.default_rng(1).standard_normal(3 * rate)
    out, L, gain, valid = R.normalize(x, rate, -22.0)
    assert valid == 1 and abs(R.integrated_loudness(out, rate)[0] + 22.0) < 1e-9
    assert gain == pytest.approx(10 ** ((-22.0 - L) / 20), rel=1e-15)


def test_peak_guard():
    rate = 22050
    x = np.zeros(2 * rate)
    x[::50] = 0.9                                   # sparse clicks: little loudness, a high peak
    plain, L, g0, _ = R.normalize(x, rate, -10.0, peak_limit=False)
    assert np.max(np.abs(plain)) > 1.0
    out, L2, g1, valid = R.normalize(x, rate, -10.0, peak_limit=True)
    assert L2 == L and valid == 1 and np.max(np.abs(out)) == pytest.approx(1.0, abs=1e-15) and g1 == pytest.approx(1 / 0.9, rel=1e-15)
    assert R.integrated_loudness(out, rate)[0] < -10.0


@pytest.mark.parametrize("rate", [48000, 22050, 16000, 11025])
def test_host_design_of_the_package_equals_the_restatement(rate):
    import ctts_amd
    from ctts_amd import loudness as LD
    for (b, a), (rb, ra) in zip(LD.kweighting(rate), R.kweighting(rate)):
        assert np.array_equal(b, rb) and np.array_equal(a, ra) and b.dtype == np.float64
    assert ctts_amd.kweighting is LD.kweighting
    # the state-transition matrix: zero-input response of lfilter from a state = powers of A
    (sb, sa), (hb, ha) = LD.kweighting(rate)
    A = LD.state_transition(rate)
    s0 = np.array([0.3, -0.2, 0.5, 0.1])
    u, zf = lfilter(sb, sa, np.zeros(300), zi=s0[:2])
    _, zf2 = lfilter(hb, ha, u, zi=s0[2:])
    want = np.concatenate([zf, zf2])
    got = np.linalg.matrix_power(A, 300) @ s0
    # the high pass has a double pole (Q = 0.5): rounding grows like n^2 2^-53 over n steps, 300^2 2^-53 = 1e-11 in both evaluations
    assert np.max(np.abs(got - want)) <= 1e-9 * np.max(np.abs(want))
    for n in (1, 100000):
        assert LD.n_blocks(n * 7 + int(0.4 * rate), rate) == R.n_blocks(n * 7 + int(0.4 * rate), rate)


@pytest.mark.parametrize("rate", [48000, 22050, 16000, 11025])
@pytest.mark.parametrize("window", ["momentary", "short_term"])
def test_block_tables_cut_where_the_restatement_cuts(rate, window):
    from ctts_amd import loudness as LD, kernels as K
    t_g, step = LD.WINDOWS[window]
    assert (t_g, step) == {"momentary": (R.T_MOMENTARY, R.STEP_MOMENTARY), "short_term": (R.T_SHORT_TERM, R.STEP_SHORT_TERM)}[window]
    n = 7 * rate + 13
    edges, chunk_seg, blocks = LD.block_tables(rate, window, n)
    chunk, slots = K.loudness_chunk(), K.loudness_limits()[0]
    assert edges[0] == 0 and edges[-1] == 2 ** 31 - 1 and np.all(np.diff(edges.astype(np.int64)) > 0)
    assert len(blocks) >= R.n_blocks(n, rate, t_g, step)
    for j, (k0, k1) in enumerate(blocks):
        assert (edges[k0], edges[k1]) == R.block_bounds(j, rate, t_g, step)
    assert len(chunk_seg) % 64 == 0 and len(chunk_seg) * chunk >= n
    for c in (0, 1, 17, len(chunk_seg) - 1):
        assert edges[chunk_seg[c]] <= c * chunk < edges[chunk_seg[c] + 1]
    last = np.searchsorted(edges, (np.arange(len(chunk_seg) // 64) + 1) * 64 * chunk - 1, side="right") - 1
    assert np.max(last - chunk_seg[::64]) < slots
    # counted from sample 0: the tables of a longer row extend those of a shorter one
    e2, c2, b2 = LD.block_tables(rate, window, 3 * n)
    assert np.array_equal(c2[:len(chunk_seg)], chunk_seg) and np.array_equal(b2[:len(blocks)], blocks)
