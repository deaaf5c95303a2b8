"""GPU: the mel front end - the one-launch FFT kernel (csrc/mel.hip) and the DFT-as-GEMM path (reflect_pad, stft_magnitude and
log_clamp_transpose of csrc/elementwise.hip around two GEMMs) - against the independent model tests/mel_restate.py in float64, over the
filterbanks, signals, lengths, hops and FFT sizes at which the launch arithmetic takes another path
(tests/test_mel_restate_cpu.py::test_case_list_reaches_every_path_of_the_fft_kernel holds the table).

Error measure, per frame and never the tensor's global maximum (s_f = float64 energy of frame f):
  mag     |mag - mag64| / s_f per bin            energy  |e - e64| / s_f
  mel     |max(exp(mel), clip) - max(mel_lin64, clip)| / (||basis[n]||_2 s_f + |ref|)   (the clamp is 1-Lipschitz: no element is left
          out around the clip; |ref| carries the rounding of logf / exp)
A frame with s_f = 0 must give energy exactly 0 and every mel bit-equal to float32 log(clip); the columns f >= Fb of a ragged row must be
bit-equal to column Fb - 1.  No element is excluded from any comparison.
Bar of every quantity: max(TWIN_X x the float32 twin under the same measure on the same input, FLOOR).  The twin is the reference
project's formulation (windowed DFT-basis product, float32 filterbank product) in float32 on the CPU.  TWIN_X = 3 is the rule of
tests/test_pitch_features_gpu.py and FLOOR = 4 * 2^-23 the floor of tests/test_seq_kernels_gpu.py: both INHERITED, neither taken from
these kernels.  Both paths are held to the same bar.  Every comparison prints `kernel / twin / bar` (run with -s).

WIDER (below, each entry with its measured ratio and its reason) replaces FLOOR for three quantities, by a floor reasoned from the
arithmetic and not from the kernel's figures:
  mag, energy on the DFT-as-GEMM path   sqrt(3 n_fft / 4) * 2^-24 (1.65e-6 at n_fft 1024): the GEMM adds the n_fft products of a bin in
      n_fft / 4 MFMA steps in program order.  For a pure tone every product has one sign, each step rounds a partial sum of the size of
      |X| <= s_f by up to 2^-24 of it, and the roundings walk: standard deviation <= sqrt(n_fft / 12) * 2^-24, the floor is three of
      them.  The twin's BLAS adds in blocks.  Measured on tones: 3.1 x (off-centre) and 4.8 x (bin 512) the twin; noise stays below 2 x.
  log_clamp_transpose called on its own   2 ulp of the float32 log at the case's largest |log|: the device logf is good to 2 ulp, numpy's
      log is correctly rounded, so 3 x the twin allows only 1.5 ulp.  Measured 1.86 ulp near log = -10.  Inside the front end the
      measure's s_f term covers it and no widening is needed.  log(clip) itself is exact in both paths (computed on the host in double).

Paths reached (tests/test_mel_restate_cpu.py asserts the table): keep_low false (40 / 0-4000, 17 / 300-5400, 96 / 0-1500, mod0/4/28 with
their own kmax), MS 73 .. 257, 373, 513 and 517 (by kmax 0 and by weight on bin 512), one to six filter tiles, partial last tiles, an
empty tile, klo 12 and 92 on tile 0, last K groups of 0, 1 and 7 steps, 1 .. 5 trips of the persistent loop (grid 3 in a child process),
hops 64 .. 1100 (unaligned frames, a zero-padded window, samples no frame loads), n_fft 512 / 1024 / 2048 on the GEMM path with row
strides 128, 275, 300 and 512 - every one computed, none refused.

Measured on the MI355X, worst case per quantity and path by its share of the bar (kernel / twin / bar; 399 comparisons, none above 0.93
of its bar):
  mag     FFT kernel   1.3e-7 / 2.9e-7 / 8.8e-7 (off-centre tone)          DFT-GEMM  9.0e-7 / 2.9e-7 / 1.7e-6 (off-centre tone; WIDER)
  energy  FFT kernel   1.4e-7 / 1.4e-7 / 4.8e-7 (glide beside noise)       DFT-GEMM  7.3e-7 / 2.7e-7 / 1.7e-6 (bin-centred tone; WIDER)
  mel     FFT kernel   2.9e-7 / 1.5e-7 / 4.8e-7 (mod4 bank, kmax 164)      DFT-GEMM  5.9e-7 / 2.8e-7 / 8.4e-7 (dense bank)
  direct  stft_magnitude 2.1e-8 / 2.1e-8 / 4.8e-7 (mag), 2.2e-8 / 2.2e-8 / 4.8e-7 (energy); log_clamp_transpose 1.8e-6 / 5.0e-7 / 1.9e-6
          ([2, 37, 80]; WIDER); reflect_pad bit-exact
  bit-exact  zero frames (energy 0, mel = float32 log(clip)), ragged columns past Fb, NaN / 7.0 padding against zero padding, grid 3
          against the full grid
Before the fixes of this change 27 of these tests failed: every swapped-filterbank case on both paths (mel up to 0.44 of the measure
instead of 8e-7: the old filters, or the old kmax on the new filters), the range contract at hop 600 and 1100 (a sample above 1 in the
unread tail raised nothing), and every signal with a frame of exact zeros (mel two float32 steps from log(clip)).
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ctts_amd
from ctts_amd import kernels as K
from tests import mel_cases as C
from tests import mel_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN_X = 3.0
FLOOR = 4 * 2.0 ** -23
CLIP = 1e-5
LOG_CLIP32 = np.log(np.float32(CLIP))



def _coherent_sum_floor(n_fft):
    """3 sigma of n_fft / 4 independent fp32 roundings of a partial sum no larger than the frame's energy: sqrt(3 n_fft / 4) * 2^-24"""
    return math.sqrt(3 * n_fft / 4) * 2.0 ** -24


# (quantity, path) -> what replaces FLOOR for it, with the measured ratio to the twin and the reason
WIDER = {
    ("mag", "dft"): dict(floor=_coherent_sum_floor, measured="4.8 x the twin (8.0e-7 against 1.7e-7, tone at bin 512); 3.1 x on an off-centre tone",
                         reason="the GEMM adds the n_fft products of a bin in n_fft / 4 MFMA steps in program order; for a pure tone they all "
                                "have one sign, every step rounds a partial sum of the size of |X|, and the roundings walk; the twin's BLAS "
                                "adds in blocks"),
    ("energy", "dft"): dict(floor=_coherent_sum_floor, measured="17 x the twin (6.9e-7 against 4.0e-8, tone at bin 512), 1.45 x FLOOR",
                            reason="the energy of a pure tone is its one bin: the same walk; the twin happens to be nearly exact there"),
    ("mel", "log_clamp_transpose"): dict(floor=lambda max_abs_log: 2 * 2.0 ** (math.floor(math.log2(max_abs_log)) - 23),
                                         measured="3.5 x the twin (1.8e-6 against 5.0e-7 on 5920 values between 1e-5 and 256): 1.86 ulp of a "
                                                  "float32 near -10",
                                         reason="called on its own the kernel shows the device logf alone, which is good to 2 ulp of its float32 "
                                                "result; numpy's log is correctly rounded (0.5 ulp), so 3 x the twin allows 1.5 ulp.  The floor is "
                                                "2 ulp at the largest |log| of the case.  Inside the front end the measure's s_f term covers it"),
}


def bar_of(q, path, twin, n_fft):
    w = WIDER.get((q, path))
    return max(TWIN_X * twin, FLOOR if w is None else w["floor"](n_fft))
N0 = 256 * 16 + 37
NEXT1 = float(np.nextafter(np.float32(1), np.float32(2)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(tag, path, got, y, lens, cfg, basis):
    """got = (mag [B, F, nbins] or None, energy [B, F], mel [B, n_mel, F]) device tensors, held to the bar against float64"""
    mag, energy, mel = [None if t is None else t.detach().cpu().numpy() for t in got]
    ref = R.mel_frontend(y, lens, *cfg, basis, clip=CLIP)
    tw = R.mel_frontend(y, lens, *cfg, basis, clip=CLIP, dtype=np.float32)
    assert energy.shape == ref[1].shape and mel.shape == ref[3].shape and (mag is None or mag.shape == ref[0].shape), (tag, mel.shape, ref[3].shape)
    assert energy.dtype == mel.dtype == np.float32
    assert np.isfinite(energy).all() and np.isfinite(mel).all() and (mag is None or np.isfinite(mag).all()), tag
    m_k = R.measures((mag, energy, mel), ref, basis, CLIP)
    m_t = R.measures((tw[0] if mag is not None else None, tw[1], tw[3]), ref, basis, CLIP)
    for q in m_k:
        bar = bar_of(q, path, m_t[q], cfg[0])
        print(f"MEL| {q} | {path} | {tag} | kernel {m_k[q]:.2e} / twin {m_t[q]:.2e} / bar {bar:.2e}")
    for q in m_k:
        bar = bar_of(q, path, m_t[q], cfg[0])
        assert math.isfinite(m_k[q]) and m_k[q] <= bar, f"{q} [{path} {tag}]: kernel {m_k[q]:.3e} > bar {bar:.3e} (twin {m_t[q]:.3e})"
    silent = ref[1] == 0                                   # [B, F]
    if silent.any():
        assert not energy[silent].any(), f"{tag}: a frame of exact zeros has energy {np.abs(energy[silent]).max()}"
        cols = np.broadcast_to(silent[:, None, :], mel.shape)
        assert np.array_equal(mel[cols].view(np.uint32), np.full(int(cols.sum()), LOG_CLIP32, dtype=np.float32).view(np.uint32)), \
            f"{tag}: mel of a frame of exact zeros is not float32 log(clip) bit for bit"
        assert mag is None or not mag[silent].any()
    if lens is not None:
        F, _, fb = R.frame_counts(y.shape[1], lens, cfg[0], cfg[1], y.shape[0])
        for b in range(y.shape[0]):
            for f in range(int(fb[b]), F):
                assert np.array_equal(mel[b, :, f].view(np.uint32), mel[b, :, fb[b] - 1].view(np.uint32)) and \
                    energy[b, f].view(np.uint32) == energy[b, fb[b] - 1].view(np.uint32), (tag, b, f)
    return mel, energy, mag


def module(cfg, bank, use_fft=None):
    st = ctts_amd.TacotronSTFT(cfg[0], cfg[1], cfg[2], bank[0], C.SR, bank[1], bank[2]).to(DEV)
    if use_fft is not None:
        assert st.use_fft or not use_fft
        st.use_fft = use_fft
    return st


def run_module(st, y):
    yd = dev(y)
    mel, energy = st.mel_spectrogram(yd)
    return st.magnitudes(yd).transpose(1, 2).contiguous(), energy, mel


def run_direct(basis, y, hop=256, win=1024, kmax=0, lens=None, flag=None, ws=None):
    """the kernel through K.mel_prepare / K.mel_spectrogram_fft, magnitudes included"""
    ws = K.mel_prepare(dev(basis), 1024) if ws is None else ws
    window = dev(R.analysis_window(1024, win).astype(np.float32))
    B, N = y.shape
    mel, energy, mag = K.mel_spectrogram_fft(y if torch.is_tensor(y) else dev(y), window, ws, 1024, hop, basis.shape[0], clip=CLIP, want_mag=True,
                                             kmax=kmax, lens=None if lens is None else dev(np.asarray(lens, dtype=np.int32)), range_flag=flag)
    return mag.view(B, 1 + N // hop, 516)[:, :, :513], energy, mel


STD = (1024, 256, 1024)
BANK0 = (80, 0, 8000)


# ---- filterbanks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fft", "dft"])
@pytest.mark.parametrize("bank", C.REAL_BANKS, ids=C.bank_name)
def test_real_filterbanks_through_the_module(bank, path):
    y = C.signal("noise", 2, N0)
    st = module(STD, bank, path == "fft")
    basis = C.filterbank(bank)
    assert np.array_equal(st.mel_basis.cpu().numpy(), basis)
    assert st._kmax == R.kmax_of(basis)
    check(C.bank_name(bank), path, run_module(st, y), y, None, STD, basis)


@pytest.mark.parametrize("kmax", ["own", 0])
@pytest.mark.parametrize("bank", C.SYNTHETIC_BANKS)
def test_synthetic_filterbanks_through_the_kernel_entry_points(bank, kmax):
    y = C.signal("noise", 2, N0, seed=1)
    basis = C.filterbank(bank)
    k = R.kmax_of(basis) if kmax == "own" else 0
    check(f"{bank} kmax {k}", "fft", run_direct(basis, y, kmax=k), y, None, STD, basis)


def test_a_kmax_below_the_filterbank_is_never_a_wrong_mel():
    """the kmax contract (include/ctts.h): a launch whose kmax is smaller than the reach of the workspace's filterbank gives NaN for the
    filters of the tiles that reach further, raises the flag with CTTS_MEL_FLAG_KMAX, and leaves every other tile and the energy right"""
    y = C.signal("noise", 2, N0, seed=2)
    basis = C.filterbank(BANK0)
    t = R.bank_table(basis)
    kmax = 200                                             # MS 201: tiles whose khi > 200 are short
    short = [i for i, (lo, hi) in enumerate(t["kr"]) if hi > R.row_stride(kmax) - 1]
    assert short and len(short) < t["tiles"]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    mag, energy, mel = run_direct(basis, y, kmax=kmax, flag=flag)
    assert int(flag.item()) & 0xFFFFFFFF == 0x7FC0004B
    mel = mel.cpu().numpy()
    rows = np.zeros(80, dtype=bool)
    for i in short:
        rows[16 * i:16 * i + 16] = True
    assert np.isnan(mel[:, rows]).all() and np.isfinite(mel[:, ~rows]).all()
    keep = basis[~rows]
    check("kmax 200 of 372, whole tiles", "fft", (mag, energy, torch.from_numpy(mel[:, ~rows])), y, None, STD, keep)
    st = module(STD, BANK0)                                # the module reports it as an error of its own, not as a range violation
    host, ev = st._range_state(DEV)
    K.mel_spectrogram_fft(dev(y), st._window, st._workspace(), 1024, 256, 80, kmax=kmax, range_flag=host)
    ev.record()
    with pytest.raises(RuntimeError, match="kmax"):
        st.check_range()


# ---- signals -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fft", "dft", "fft 40mel_0_4000"])
@pytest.mark.parametrize("name", C.SIGNALS)
def test_signals(name, path):
    bank = BANK0 if path in ("fft", "dft") else (40, 0, 4000)          # the second bank keeps bins 256 and 512 out of the tile
    y = C.signal(name, 2, N0)
    st = module(STD, bank, path != "dft")
    check(name, path, run_module(st, y), y, None, STD, C.filterbank(bank))


# ---- lengths -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fft", "dft"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [513, 700, 256 * 16 - 1, 256 * 16, 4133])
def test_lengths(N, B, path):
    """odd N with B > 1: every other row starts misaligned for the 8-byte pair loads"""
    y = C.signal("noise", B, N, seed=N)
    st = module(STD, BANK0, path == "fft")
    check(f"N {N} B {B}", path, run_module(st, y), y, None, STD, C.filterbank(BANK0))


@pytest.mark.parametrize("fill", [float("nan"), 7.0])
def test_ragged_lens_against_the_model(fill):
    """the padding past lens[b] is never read: bit-equal to the zero-padded run, range flag down, and right against float64"""
    N = N0
    lens = [513, 514, 256 * 15 + 255, 256 * 16, N]
    y = C.signal("noise", len(lens), N, seed=7)
    for b, n in enumerate(lens):
        y[b, n:] = 0.0
    junk = y.copy()
    for b, n in enumerate(lens):
        junk[b, n:] = fill
    basis = C.filterbank(BANK0)
    ws = K.mel_prepare(dev(basis), 1024)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    clean = run_direct(basis, y, kmax=372, lens=lens, ws=ws)
    got = run_direct(basis, junk, kmax=372, lens=lens, flag=flag, ws=ws)
    assert int(flag.item()) == 0
    for a, b_ in zip(got, clean):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32))
    check(f"ragged fill {fill}", "fft", got, y, lens, STD, basis)
    st = module(STD, BANK0)                                # the preprocessing entry point: per-utterance results
    outs = st.mel_spectrograms_ragged([y[b, :n] for b, n in enumerate(lens)])
    for b, (n, (mel, en)) in enumerate(zip(lens, outs)):
        fb = 1 + n // 256
        assert np.array_equal(mel, got[2][b, :, :fb].cpu().numpy()) and np.array_equal(en, got[1][b, :fb].cpu().numpy())


# ---- hops (FFT kernel) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,win", [(64, 1024), (200, 800), (256, 1024), (275, 1024), (600, 1024), (1024, 1024), (1100, 1024)])
def test_hops(hop, win):
    """odd hops take the unaligned load path on every other frame; win 800 is zero-padded inside the frame; hop > n_fft leaves samples
    between the frames that only the range check reads"""
    y = C.signal("noise", 2, 4000, seed=hop)
    cfg = (1024, hop, win)
    check(f"hop {hop} win {win}", "fft", run_module(module(cfg, BANK0, True), y), y, None, cfg, C.filterbank(BANK0))


# ---- other sizes (DFT-as-GEMM path) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(2048, 300, 1200), (2048, 512, 2048), (512, 128, 512), (1024, 275, 1024)], ids=str)
def test_other_fft_sizes_on_the_dft_gemm_path(cfg):
    y = C.signal("noise", 2, 5000, seed=cfg[1])
    st = module(cfg, BANK0, False)
    basis = ctts_amd.audio.slaney_mel_basis(C.SR, cfg[0], 80, 0, 8000)
    assert not st.use_fft and np.array_equal(st.mel_basis.cpu().numpy(), basis)
    check(f"n_fft {cfg[0]} hop {cfg[1]} win {cfg[2]}", "dft", run_module(st, y), y, None, cfg, basis)


def test_elementwise_kernels_at_one_row_one_frame_one_filter():
    rng = np.random.RandomState(5)
    # reflect_pad: one row, exact
    for N, pad in [(2, 1), (5, 4), (513, 512), (1030, 1024)]:
        y = rng.uniform(-1, 1, size=(1, N)).astype(np.float32)
        out = K.reflect_pad(dev(y), pad).cpu().numpy()
        ld = (N + 2 * pad + 3) // 4 * 4
        want = np.zeros((1, ld), dtype=np.float32)
        want[:, :N + 2 * pad] = np.pad(y, ((0, 0), (pad, pad)), mode="reflect")
        assert out.shape == (1, ld) and np.array_equal(out, want), (N, pad)
    # stft_magnitude: one frame; nbins 1, 513 and 1025, rows wider than nbins zero-filled
    for nbins, ld in [(1, 4), (513, 516), (1025, 1028)]:
        reim = rng.uniform(-1, 1, size=(1, 2 * nbins)).astype(np.float32)
        mag, energy = K.stft_magnitude(dev(reim), 1, nbins, ld)
        mag, energy = mag.cpu().numpy(), energy.cpu().numpy()
        re, im = reim[:, :nbins].astype(np.float64), reim[:, nbins:].astype(np.float64)
        m64 = np.sqrt(re * re + im * im)
        s = np.sqrt((m64 ** 2).sum())
        m32 = np.sqrt(reim[:, :nbins] ** 2 + reim[:, nbins:] ** 2)
        e32 = np.sqrt((m32 * m32).sum(dtype=np.float32))
        assert not mag[:, nbins:].any()
        for q, k, t in [("mag", np.abs(mag[:, :nbins] - m64).max() / s, np.abs(m32 - m64).max() / s),
                        ("energy", abs(float(energy[0]) - s) / s, abs(float(e32) - s) / s)]:
            bar = max(TWIN_X * t, FLOOR)
            print(f"MEL| {q} | stft_magnitude | nbins {nbins} | kernel {k:.2e} / twin {t:.2e} / bar {bar:.2e}")
            assert k <= bar, (q, nbins, k, bar)
    # log_clamp_transpose: one frame of one filter, below, at and above the clip; and a [2, 3, 5] transpose
    for shape in [(1, 1, 1), (2, 3, 5), (2, 37, 80)]:
        B, F, n = shape
        x = (rng.uniform(0, 2, size=(B * F, n)) ** 8).astype(np.float32)             # 0 .. 256, a third of them below 1e-3
        x.flat[0] = 0.0
        for v in (x, np.full_like(x, CLIP), np.full_like(x, 3.0)):
            out = K.log_clamp_transpose(dev(v), B, F, n, CLIP).cpu().numpy()
            ref = np.maximum(v.astype(np.float64), CLIP).reshape(B, F, n).transpose(0, 2, 1)
            t32 = np.log(np.maximum(v, np.float32(CLIP))).reshape(B, F, n).transpose(0, 2, 1)
            k = (np.abs(np.exp(out.astype(np.float64)) - ref) / ref).max()
            t = (np.abs(np.exp(t32.astype(np.float64)) - ref) / ref).max()
            bar = max(TWIN_X * t, FLOOR, WIDER[("mel", "log_clamp_transpose")]["floor"](float(np.abs(np.log(ref)).max())))
            print(f"MEL| mel | log_clamp_transpose | {shape} | kernel {k:.2e} / twin {t:.2e} / bar {bar:.2e}")
            assert out.shape == (B, n, F) and k <= bar, (shape, k, bar)


# ---- the persistent loop -------------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys
import numpy as np, torch
import ctts_amd
from ctts_amd import kernels as K
y = torch.from_numpy(np.load(sys.argv[1])).cuda()
st = ctts_amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).cuda()
mel, energy, mag = K.mel_spectrogram_fft(y, st._window, st._workspace(), 1024, 256, 80, want_mag=True, kmax=st._kmax)
torch.cuda.synchronize()
np.savez(sys.argv[2], mel=mel.cpu().numpy(), energy=energy.cpu().numpy(), mag=mag.cpu().numpy())
print("CHILD OK")
"""


def test_persistent_loop_with_three_workgroups_in_a_child_process(tmp_path):
    """15 tiles on a grid of 3 (CTTS_MEL_GRID is read once per process, hence the child): five trips per workgroup, every value of the
    role rotation, a trip that crosses a batch boundary - bit-equal to this process's full-grid run and within the bar of float64"""
    B, N = 3, 256 * 70 + 11
    y = C.signal("noise", B, N, seed=70)
    assert B * ((1 + N // 256 + 15) // 16) == 15
    np.save(tmp_path / "y.npy", y)
    env = dict(os.environ, CTTS_MEL_GRID="3", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "y.npy"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    child = np.load(tmp_path / "out.npz")
    assert "CTTS_MEL_GRID" not in os.environ
    st = module(STD, BANK0)
    mel, energy, mag = K.mel_spectrogram_fft(dev(y), st._window, st._workspace(), 1024, 256, 80, want_mag=True, kmax=st._kmax)
    for name, t in (("mel", mel), ("energy", energy), ("mag", mag)):          # mag rows are 516 wide, the kernel writes 513 bins
        a, b_ = (child[name], t.cpu().numpy()) if name != "mag" else (child[name][:, :513], t.cpu().numpy()[:, :513])
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b_).view(np.uint32)), name
    F = 1 + N // 256
    got = (torch.from_numpy(child["mag"]).view(B, F, 516)[:, :, :513], torch.from_numpy(child["energy"]), torch.from_numpy(child["mel"]))
    check("grid 3, 15 tiles", "fft", got, y, None, STD, C.filterbank(BANK0))


# ---- the range contract --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,N", [(256, N0), (600, 600 * 6 + 590), (1100, 1100 * 3 + 700)])
def test_range_contract_over_the_whole_waveform(hop, N):
    """exactly +-1.0 everywhere is inside; the next float above 1, or a NaN, anywhere is not: the first sample, the reflected regions,
    the last sample, the tail N % hop (which no frame loads when it is longer than n_fft/2) and the gap between frames of hop > n_fft"""
    st = module((1024, hop, 1024), BANK0)
    rng = np.random.RandomState(hop)
    y = np.where(rng.rand(2, N) < 0.5, -1.0, 1.0).astype(np.float32)
    st.mel_spectrogram(dev(y))                             # raises nothing
    F = 1 + N // hop
    tail = (F - 1) * hop + (N % hop + 512) // 2            # for a tail longer than 512: past the last frame's last sample
    places = {"first": 0, "reflected head": 100, "reflected tail": N - 100, "last": N - 1, "tail": min(tail, N - 1)}
    if hop > 1024:
        places["gap"] = hop + 512 + (hop - 1024) // 2
    if N % hop > 512:
        assert (F - 1) * hop + 512 <= places["tail"] < N - 1                                                  # no frame loads it
    for what, p in places.items():
        for b in range(2):
            for v in (NEXT1, -NEXT1, float("nan")):
                bad = y.copy()
                bad[b, p] = v
                with pytest.raises(AssertionError):
                    st.mel_spectrogram(dev(bad))
                    pytest.fail(f"hop {hop}: {v} at sample {p} ({what}) of row {b} raised nothing", pytrace=False)
    st.mel_spectrogram(dev(y))                             # the flag was cleared


# ---- the filterbank is the module's state --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["copy_", "load_state_dict", "set_mel_basis"])
@pytest.mark.parametrize("when", ["before the first call", "after a first call"])
@pytest.mark.parametrize("path", ["fft", "dft"])
def test_a_swapped_filterbank_is_the_one_both_paths_use(path, when, how):
    """mel_basis.copy_(...), load_state_dict and set_mel_basis replace the 80 / 0-8000 bank (kmax 372) by the dense one (weight on every
    bin up to 512): the padded copy of the DFT path, the FFT kernel's workspace and its kmax all follow"""
    y = C.signal("noise", 2, N0, seed=3)
    st = module(STD, BANK0, path == "fft")
    if when == "after a first call":
        check("before the swap", path, run_module(st, y), y, None, STD, C.filterbank(BANK0))
    dense = C.filterbank("dense")
    if how == "copy_":
        st.mel_basis.copy_(dev(dense))
    elif how == "load_state_dict":
        assert list(st.state_dict()) == ["mel_basis"]
        st.load_state_dict({"mel_basis": torch.from_numpy(dense)})
    else:
        st.set_mel_basis(dense)
    check(f"dense after {how}, {when}", path, run_module(st, y), y, None, STD, dense)
    assert st._kmax == 513
    st.mel_basis.copy_(dev(C.filterbank(BANK0)))           # and back: a smaller kmax again
    check(f"back after {how}, {when}", path, run_module(st, y), y, None, STD, C.filterbank(BANK0))
    assert st._kmax == 372


def test_a_swapped_filterbank_is_not_rebuilt_inside_a_graph_capture(monkeypatch):
    st = module(STD, BANK0)
    y = dev(C.signal("noise", 1, 2048))
    st.magnitudes(y)
    st.mel_basis.copy_(dev(C.filterbank("dense")))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before capturing a graph"):
        st.magnitudes(y)
    monkeypatch.undo()
    st.magnitudes(y)
    assert st._kmax == 513
