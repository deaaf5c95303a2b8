"""CPU: pins tests/mel_restate.py, the independent model that tests/test_mel_kernels_gpu.py holds the mel kernels to - against the
reference's own recorded output (G8), against closed forms of the hann-windowed DFT, against torch's reflect padding, and against six
plausible misreadings of the front end, each of which must miss by a printed margin.  The last tests restate the launch table of the FFT
kernel (kmax, row stride MS, keep_low, per-tile bin ranges) from the filterbank arrays and assert that the case list of the GPU module
reaches every path the kernel has.  Run with -s for the figures."""
import numpy as np
import pytest
import torch

from tests import mel_cases as C
from tests import mel_restate as R
from tests.util import load_golden

FLOOR = 4 * 2.0 ** -23                 # the floor of the GPU module's bar: a misreading must miss it by orders of magnitude
CFG = (1024, 256, 1024)
BASIS = C.filterbank((80, 0, 8000))


def test_model_reproduces_the_reference_golden():
    """G8 is the reference's own TacotronSTFT output (float32 conv1d arithmetic).  The float64 model is as far from it as
    tests/test_kernels_gpu.py measures the reference to be from float64 (|X| and energy 2e-5 of full scale, linear mel 1e-5 of full scale,
    log-mel 1e-3 on bins above 1e-3 and 2e-3 on all bins: 1.75e-3 measured there, on near-silent bins whose float32 rounding the log
    amplifies).  The float32 twin is a second float32 evaluation of the same formulation with its own summation order: on all bins it may
    be twice that away, 4e-3, the bound tests/test_kernels_gpu.py sets for the kernels against G8."""
    g = load_golden("g8_stft")
    assert np.array_equal(g["mel_basis"], BASIS) or np.abs(g["mel_basis"] - BASIS).max() <= 1e-6
    for dtype in (np.float64, np.float32):
        mag, energy, lin, log = R.mel_frontend(g["y"], None, *CFG, g["mel_basis"], dtype=dtype)
        assert log.shape == g["mel"].shape and energy.shape == g["energy"].shape and mag.shape == (2, 87, 513)
        gm = g["mag"].transpose(0, 2, 1).astype(np.float64)
        e_mag = np.abs(mag - gm).max() / max(1.0, gm.max())
        e_en = np.abs(energy - g["energy"]).max() / max(1.0, g["energy"].max())
        ref = g["mel"].astype(np.float64)
        loud = np.exp(ref) > 1e-3
        e_loud = np.abs(log - ref)[loud].max()
        e_all = np.abs(log - ref).max()
        e_lin = np.abs(np.maximum(lin, 1e-5) - np.exp(ref)).max() / np.exp(ref).max()
        print(f"G8 vs model {np.dtype(dtype).name}: |X| {e_mag:.2e}  energy {e_en:.2e}  log-mel loud {e_loud:.2e} all {e_all:.2e}  linear mel {e_lin:.2e}")
        assert e_mag <= 2e-5 and e_en <= 2e-5 and e_loud <= 1e-3 and e_all <= (2e-3 if dtype == np.float64 else 4e-3) and e_lin <= 1e-5


def test_float32_twins_against_float64_on_noise():
    """the twin's own distance from float64 under the GPU module's measures, and scipy's float32 rFFT beside it (information)"""
    y = C.signal("noise", 2, 256 * 16 + 37)
    ref = R.mel_frontend(y, None, *CFG, BASIS)
    tw = R.mel_frontend(y, None, *CFG, BASIS, dtype=np.float32)
    sp = R.mel_frontend_scipy32(y, None, *CFG, BASIS)
    assert all(a.dtype == np.float32 for a in tw) and all(a.dtype == np.float64 for a in ref)
    m_tw, m_sp = R.measures((tw[0], tw[1], tw[3]), ref, BASIS), R.measures((sp[0], sp[1], sp[3]), ref, BASIS)
    print(f"float32 twin (DFT basis product) vs float64: {m_tw}\nfloat32 scipy rFFT vs float64: {m_sp}")
    for m in (m_tw, m_sp):
        assert 0 < m["mag"] <= 1e-6 and m["energy"] <= 1e-6 and m["mel"] <= 1e-6
    same = R.measures((ref[0], ref[1], ref[3]), ref, BASIS)           # exp(log(x)) in float64: one rounding
    assert same["mag"] == 0.0 and same["energy"] == 0.0 and same["mel"] <= 2.0 ** -50


def _interior(N, hop=256, n_fft=1024):
    return [f for f in range(1 + N // hop) if f * hop >= n_fft // 2 and f * hop + n_fft // 2 <= N]


def test_closed_forms_of_the_hann_windowed_dft():
    N, A = 256 * 16 + 37, 0.7
    n = np.arange(N, dtype=np.float64)
    one = np.ones((1, 513), dtype=np.float32)              # a one-filter bank: mel_lin = sum of |X|
    tol = 1e-9

    def mags(y):
        return R.mel_frontend(y[None], None, *CFG, one)

    # a constant: bins 0 and 1 only, at every frame (the reflection of a constant is the constant)
    mag, energy, lin, log = mags(np.full(N, 0.5))
    assert np.abs(mag[0, :, 0] - 0.5 * 512).max() <= tol and np.abs(mag[0, :, 1] - 0.5 * 256).max() <= tol and np.abs(mag[0, :, 2:]).max() <= tol
    assert np.abs(energy[0] - 0.5 * np.hypot(512, 256)).max() <= tol and np.abs(lin[0, 0] - 0.5 * 768).max() <= 1e-7
    # a bin-centred cosine and a tone at exactly bin 256: A n_fft / 4 at the bin, half of that at both neighbours (interior frames: a
    # reflected cosine changes its phase at the edge)
    for k0 in (40, 256):
        mag = mags(A * np.cos(2 * np.pi * k0 * n / 1024 + 0.3))[0][0, _interior(N)]
        want = np.zeros(513)
        want[k0], want[k0 - 1], want[k0 + 1] = A * 256, A * 128, A * 128
        assert len(mag) >= 10 and np.abs(mag - want).max() <= tol, np.abs(mag - want).max()
    # alternating +-1: bin 512 (n_fft / 2) and its one neighbour 511, at every frame (both reflections keep the parity)
    mag = mags(np.cos(np.pi * n))[0][0]
    want = np.zeros(513)
    want[512], want[511] = 512, 256
    assert np.abs(mag - want).max() <= tol
    # a unit impulse at sample 5 * 256: |X[k]| = w[position in the frame] for every k
    y = np.zeros(N)
    y[5 * 256] = 1.0
    mag = mags(y)[0][0]
    w = R.analysis_window(1024, 1024)
    for f in range(mag.shape[0]):
        p = 5 * 256 - (f * 256 - 512)
        assert np.abs(mag[f] - (w[p] if 0 <= p < 1024 else 0.0)).max() <= tol, f
    assert w[512] == 1.0 and w[0] == 0.0 and abs(w[256] - 0.5) <= 1e-15 and w[1] == w[1023]          # periodic: w[n] = w[n_fft - n]
    # all zeros: energy exactly 0, every mel exactly log(clip), in both precisions
    for dtype in (np.float64, np.float32):
        mag, energy, lin, log = R.mel_frontend(np.zeros((2, N)), None, *CFG, BASIS, dtype=dtype)
        assert not mag.any() and not energy.any() and not lin.any() and np.array_equal(log, np.full(log.shape, np.log(dtype(1e-5)), dtype=dtype))
    assert np.log(np.float32(1e-5)).dtype == np.float32


@pytest.mark.parametrize("n_fft,hop,N", [(1024, 256, 4133), (1024, 275, 4000), (2048, 300, 5000), (512, 128, 700), (1024, 600, 513)])
def test_framing_equals_torch_reflect_padding(n_fft, hop, N):
    y = C.signal("noise", 3, N)
    F = 1 + N // hop
    pad = torch.nn.functional.pad(torch.from_numpy(y)[:, None], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
    want = pad.unfold(1, n_fft, hop).numpy()
    got = R.frame_matrix(y, None, n_fft, hop)
    assert got.shape == want.shape == (3, F, n_fft) and np.array_equal(got, want)
    # ragged: every utterance on its own, reflected at its own end; later frames of the row repeat its last frame
    lens = [N, n_fft // 2 + 1, max(n_fft // 2 + 1, N - hop - 3)]
    junk = y.copy()
    for b, n in enumerate(lens):
        junk[b, n:] = 7.0
    got = R.frame_matrix(junk, lens, n_fft, hop)
    for b, n in enumerate(lens):
        fb = 1 + n // hop
        one = torch.nn.functional.pad(torch.from_numpy(y[b, :n])[None, None], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
        want = one.unfold(0, n_fft, hop).numpy()
        assert want.shape[0] == fb and np.array_equal(got[b, :fb], want)
        assert all(np.array_equal(got[b, f], want[fb - 1]) for f in range(fb, F))


MISREAD_INPUTS = {
    # misreading -> (n_fft, hop, win), N, lens, what the input needs
    "symmetric_window": ((1024, 256, 1024), 4133, None),
    "zero_padding": ((1024, 256, 1024), 4133, None),
    "frames_n_over_hop": ((1024, 256, 1024), 4133, None),
    "uncentred_window": ((1024, 200, 800), 4000, None),                 # needs win < n_fft
    "reflect_at_row_end": ((1024, 256, 1024), 4133, [4133, 3000]),       # needs an utterance shorter than its row
    "energy_kept_bins": ((1024, 256, 1024), 4133, None),                # needs a bank that ends below Nyquist (80 / 0-8000)
}


@pytest.mark.parametrize("misread", R.MISREADINGS)
def test_each_misreading_of_the_front_end_fails_by_a_wide_margin(misread):
    cfg, N, lens = MISREAD_INPUTS[misread]
    y = C.signal("noise", 2, N, hop=cfg[1])
    if lens is not None:
        for b, n in enumerate(lens):
            y[b, n:] = 7.0
    ref = R.mel_frontend(y, lens, *cfg, BASIS)
    bad = R.mel_frontend(y, lens, *cfg, BASIS, misread=misread)
    if misread == "frames_n_over_hop":
        print(f"{misread}: {bad[3].shape[2]} frames instead of {ref[3].shape[2]}")
        assert bad[3].shape[2] == ref[3].shape[2] - 1 == N // cfg[1]
        return
    m = R.measures((bad[0], bad[1], bad[3]), ref, BASIS)
    worst = max(m.values())
    print(f"{misread}: {m}  = {worst / FLOOR:.1e} x the floor of the bar")
    assert worst >= 1e3 * FLOOR, (misread, m)
    if misread == "energy_kept_bins":
        assert m["mag"] == 0.0 and m["mel"] <= 2.0 ** -50 and m["energy"] >= 1e3 * FLOOR
    # and the same model without the misreading is the reference, bit for bit
    again = R.mel_frontend(y, lens, *cfg, BASIS)
    assert all(np.array_equal(a, b) for a, b in zip(again, ref))


# ---- the launch table of the FFT kernel over the case list -------------------------------------------------------------------------------------
def _table():
    rows = {}
    for spec in C.REAL_BANKS + C.SYNTHETIC_BANKS:
        w = C.filterbank(spec)
        rows[C.bank_name(spec)] = R.bank_table(w)
        if isinstance(spec, str):                          # synthetic banks also run with kmax = 0 (every bin kept)
            rows[C.bank_name(spec) + "/kmax0"] = R.bank_table(w, kmax=0)
    return rows


def test_launch_table_matches_what_is_stated_for_the_real_banks():
    for spec, (kmax, ms) in C.STATED.items():
        t = R.bank_table(C.filterbank(spec))
        assert t["MS"] == ms and (kmax is None or t["kmax"] == kmax), (spec, t)
    t = R.bank_table(C.filterbank((80, 2000, 11025)))
    assert t["klo0"] == 92, t
    assert R.row_stride(0) == R.row_stride(513) == 517 and R.row_stride(512) == 513 and R.row_stride(255) == 257 and R.row_stride(253) == 257
    # the bin ranges are inside the row for the bank's own kmax: the last bin read is khi - 1 <= MS - 2
    for name, t in _table().items():
        assert all(hi <= t["MS"] - 1 and lo % 4 == 0 and hi % 4 == 0 and lo <= hi for lo, hi in t["kr"]), (name, t)


def test_case_list_reaches_every_path_of_the_fft_kernel():
    rows = _table()
    for name, t in rows.items():
        print(f"{name:22s} n_mel {t['n_mel']:2d} kmax {t['kmax']:3d} MS {t['MS']:3d} keep_low {int(t['keep_low'])} tiles {t['tiles']} "
              f"empty {t['empty_tiles']} mods {t['group_mods']} kr {t['kr']}")
    reach = {
        "keep_low false": [n for n, t in rows.items() if not t["keep_low"]],
        "MS 257": [n for n, t in rows.items() if t["MS"] == 257],
        "MS 513": [n for n, t in rows.items() if t["MS"] == 513],
        "MS 517 by kmax 0": [n for n, t in rows.items() if t["MS"] == 517 and t["kmax"] == 0],
        "MS 517 by weight on bin 512": [n for n, t in rows.items() if t["MS"] == 517 and t["kmax"] == 513],
        "a (0, 0) tile": [n for n, t in rows.items() if t["empty_tiles"]],
        "klo > 0 on tile 0": [n for n, t in rows.items() if t["klo0"] > 0],
        "a partial last tile": [n for n, t in rows.items() if t["partial_last_tile"]],
        "one tile": [n for n, t in rows.items() if t["tiles"] == 1],
        "six tiles": [n for n, t in rows.items() if t["tiles"] == 6],
        "a tile for every role of the second round (tile 5)": [n for n, t in rows.items() if t["tiles"] == 6 and t["kr"][5][1] > t["kr"][5][0]],
        "mod 0": [n for n, t in rows.items() if 0 in t["group_mods"]],
        "mod 4": [n for n, t in rows.items() if 4 in t["group_mods"]],
        "mod 28": [n for n, t in rows.items() if 28 in t["group_mods"]],
        "whole groups and a partial one in one tile": [n for n, t in rows.items() if any(hi - lo > 32 and (hi - lo) % 32 for lo, hi in t["kr"])],
        "the self-paired bin 256 outside the row": [n for n, t in rows.items() if t["MS"] <= 256],
        "the self-paired bin 256 inside the row": [n for n, t in rows.items() if t["MS"] > 256],
    }
    for what, names in reach.items():
        print(f"{what}: {names}")
        assert names, f"no case reaches: {what}"
    assert {t["n_mel"] for t in rows.values()} >= {1, 16, 17, 33, 40, 80, 96}
