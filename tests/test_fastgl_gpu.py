"""GPU: fast Griffin-Lim (the momentum variant of csrc/griffinlim.hip's iteration) and the initial phase drawn on the device, through
ctts_amd.kernels and ctts_amd.audio.griffin_lim / inv_mel_spec, against the plain kernel (bitwise where the mathematics says so), the
float64 restatement tests/fastgl_restate.py and the integer restatement of the phase generator.

The float64 bar follows test_griffinlim_gpu.py: the same momentum loop at float32 on stock torch ops (StockSTFT) is run on the device,
its relative L2 distance from float64 is the algorithm's own float32 drift on that input, and the native result may be DRIFT_X times
that far from float64.  The measured pairs are printed under -s and quoted in DESIGN.md section 10."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import _lib, audio, kernels as K  # noqa: E402
import fastgl_restate as FR  # noqa: E402
import griffinlim_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DRIFT_X = 4.0
MOM = 0.99
COEF = MOM / (1.0 + MOM)


@pytest.fixture(scope="module")
def stft():
    return audio.STFT(1024, 256, 1024).to(DEV)


@pytest.fixture(scope="module")
def stock():
    return R.StockSTFT(DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _magnitudes(B, F, seed):
    rs = np.random.RandomState(seed)
    env = 2.0 / (1.0 + np.arange(513) / 30.0)
    return (rs.rand(B, 513, F) * env[None, :, None]).astype(np.float32)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _lens(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)


def _loop(stft, mag, ang, n, coef, lens=None, fill=None):
    """n iterations on the kernel wrappers: coef None = griffinlim_iter, else griffinlim_iter_momentum with the state pre-filled with
    `fill`.  Returns (waveform, state)"""
    ws = stft._workspace(mag, "magnitude")
    frames = _lens(lens)
    Y, magT = K.istft_frames(mag, ang, ws, frames, want_magT=True)
    Y2 = torch.empty_like(Y)
    state = None
    if coef is not None:
        state = K.griffinlim_state(Y.shape[0], Y.shape[1], DEV)
        state.fill_(0.0 if fill is None else fill)
    for i in range(n):
        if coef is None:
            K.griffinlim_iter(Y, magT, ws, Y2, frames)
        else:
            K.griffinlim_iter_momentum(Y, magT, state, ws, Y2, coef, i == 0, frames)
        Y, Y2 = Y2, Y
    return K.istft_ola(Y, ws, frames), state


INPUTS = {"g19": (R.g19_gl_magnitude, R.GL_SEED), "speech64": (lambda: R.speechlike_magnitude(64, 7), 11)}
_cache = {}


def _input(name):
    if name not in _cache:
        make, seed = INPUTS[name]
        mag = make()
        _cache[name] = (mag, R.seeded_angles(mag.shape, seed))
    return _cache[name]


# ---- momentum 0 and the first iteration: the plain kernel's bits
@pytest.mark.parametrize("n", [1, 4])
def test_coef_zero_is_bitwise_the_plain_iteration(stft, n):
    mag, ang = _dev(*_input("g19"))
    plain, _ = _loop(stft, mag, ang, n, None)
    zero, _ = _loop(stft, mag, ang, n, 0.0, fill=float("nan"))
    assert torch.equal(plain, zero)


def test_coef_zero_ragged_with_all_reflecting_frames(stft):
    lens = [37, 5, 4]                                       # F = 4: every frame reflects at one end at least
    mag, ang = _dev(_magnitudes(3, 37, 61), R.seeded_angles((3, 513, 37), 62))
    plain, _ = _loop(stft, mag, ang, 4, None, lens)
    zero, _ = _loop(stft, mag, ang, 4, 0.0, lens, fill=float("nan"))
    assert torch.equal(plain, zero)


def test_first_iteration_ignores_the_state(stft):
    mag, ang = _dev(*_input("g19"))
    plain, _ = _loop(stft, mag, ang, 1, None)
    fast, _ = _loop(stft, mag, ang, 1, COEF, fill=float("nan"))
    assert torch.isfinite(fast).all() and torch.equal(plain, fast)
    assert torch.equal(audio.griffin_lim(mag, stft, 1, angles=ang, momentum=MOM), audio.griffin_lim(mag, stft, 1, angles=ang))
    # and from the second iteration on the momentum term acts
    assert not torch.equal(audio.griffin_lim(mag, stft, 2, angles=ang, momentum=MOM), audio.griffin_lim(mag, stft, 2, angles=ang))


def test_momentum_zero_takes_the_plain_path(stft):
    mag, ang = _dev(*_input("g19"))
    assert torch.equal(audio.griffin_lim(mag, stft, 4, angles=ang, momentum=0.0), audio.griffin_lim(mag, stft, 4, angles=ang))


# ---- against float64
@pytest.mark.parametrize("n", [2, 4, 16])
@pytest.mark.parametrize("name", list(INPUTS))
def test_momentum_matches_fp64_within_the_float32_drift(stft, stock, name, n):
    mag, ang = _input(name)
    ref = FR.griffin_lim(mag, ang, n, MOM)
    m, a = _dev(mag, ang)
    out = audio.griffin_lim(m, stft, n, angles=a, momentum=MOM)
    assert out.shape == (1, 256 * (mag.shape[-1] - 1)) and out.dtype == torch.float32
    with torch.no_grad():
        own = R.rel_l2(_np(FR.stock_griffin_lim(stock, m, a, n, MOM)), ref)
    err = R.rel_l2(_np(out), ref)
    print(f"{name} n={n}: native rel-L2 vs float64 {err:.3e}, stock float32 momentum loop {own:.3e}")
    assert err < DRIFT_X * own


# ---- ragged batches
def test_ragged_batch_equals_per_utterance_calls_bitwise(stft):
    lens = [37, 4, 90, 64]
    B, Fmax = len(lens), max(lens)
    mag, ang = _dev(_magnitudes(B, Fmax, 31), R.seeded_angles((B, 513, Fmax), 32))
    out = audio.griffin_lim(mag, stft, 8, angles=ang, lens=lens, momentum=MOM)
    for b, F in enumerate(lens):
        L = 256 * (F - 1)
        one = audio.griffin_lim(mag[b:b + 1, :, :F], stft, 8, angles=ang[b:b + 1, :, :F], momentum=MOM)
        assert torch.equal(out[b:b + 1, :L], one), b
        assert not out[b, L:].any()


def test_ragged_batch_across_the_grid_stride_loop(stft):
    """B F = 5000 frames > the 4096 waves of a launch: some waves walk two frames, each with its own state slot"""
    lens = [1000, 517, 4, 999, 64]
    B, Fmax = len(lens), max(lens)
    mag = torch.from_numpy(_magnitudes(B, Fmax, 71)).to(DEV)
    ang = (torch.rand(B, 513, Fmax, device=DEV, generator=torch.Generator(DEV).manual_seed(72)) * 2 - 1) * np.pi
    out = audio.griffin_lim(mag, stft, 2, angles=ang, lens=lens, momentum=MOM)
    assert torch.isfinite(out).all()
    for b, F in enumerate(lens):
        L = 256 * (F - 1)
        one = audio.griffin_lim(mag[b:b + 1, :, :F], stft, 2, angles=ang[b:b + 1, :, :F], momentum=MOM)
        assert torch.equal(out[b:b + 1, :L], one), b
        assert not out[b, L:].any()


# ---- determinism and capture
def test_two_runs_and_graph_replay_with_a_seed_tensor_are_bit_identical(stft):
    lens = [100, 41, 77]
    B, Fmax = len(lens), max(lens)
    mag = torch.from_numpy(_magnitudes(B, Fmax, 41)).to(DEV)
    lens_d = _lens(lens)
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)

    def run():
        return audio.griffin_lim(mag, stft, 8, lens=lens_d, momentum=MOM, seed=seed)
    eager = run()
    assert torch.equal(eager, run())
    assert torch.equal(eager, audio.griffin_lim(mag, stft, 8, lens=lens_d, momentum=MOM, seed=1234))     # int seed = tensor seed
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                # the one warm call
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    for _ in range(2):
        captured.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
    seed.fill_(98765)                                        # the kernel reads the seed at replay time
    g.replay()
    torch.cuda.synchronize()
    other = captured.clone()
    assert torch.equal(other, audio.griffin_lim(mag, stft, 8, lens=lens_d, momentum=MOM, seed=98765))
    assert not torch.equal(other, eager)


# ---- the device phase
def test_device_phase_same_seed_same_result_other_seed_other_result(stft):
    mag = torch.from_numpy(_magnitudes(2, 40, 81)).to(DEV)
    a = audio.griffin_lim(mag, stft, 0, seed=7)
    assert a.shape == (2, 256 * 39) and torch.isfinite(a).all()
    assert torch.equal(a, audio.griffin_lim(mag, stft, 0, seed=7))
    assert torch.equal(a, audio.griffin_lim(mag, stft, 0, seed=torch.tensor([7], dtype=torch.int64, device=DEV)))
    for other in (8, 7 + (1 << 32), -7):                     # low word, high word, sign
        assert not torch.equal(a, audio.griffin_lim(mag, stft, 0, seed=other))
    assert torch.equal(audio.griffin_lim(mag, stft, 0, seed=-1), audio.griffin_lim(mag, stft, 0, seed=(1 << 64) - 1))
    with pytest.raises(_lib.CttsError):                      # the wrapper takes a device int64 only
        K.istft_frames_seeded(mag, stft._workspace(mag, "magnitude"), torch.tensor([7], dtype=torch.int64))


def test_device_phase_of_an_utterance_does_not_depend_on_the_batch(stft):
    F = 33
    m = _magnitudes(3, 50, 91)
    small = torch.from_numpy(m[:, :, :F]).to(DEV)
    big = torch.from_numpy(m).to(DEV)                        # more padding: F = 50
    for n, kw in ((0, {}), (3, {"momentum": MOM})):
        a = audio.griffin_lim(small, stft, n, seed=5, **kw)
        b = audio.griffin_lim(big, stft, n, seed=5, lens=[50, F, 8], **kw)
        c = audio.griffin_lim(big, stft, n, seed=5, lens=[4, F, 50], **kw)
        L = 256 * (F - 1)
        assert torch.equal(a[1], b[1, :L]) and torch.equal(a[1], c[1, :L]) and not b[1, L:].any()
    # b is part of the counter: the same magnitude in two rows starts from two phases
    twice = audio.griffin_lim(small[1:2].expand(2, -1, -1), stft, 0, seed=5)
    assert not torch.equal(twice[0], twice[1])
    assert torch.equal(twice[1], audio.griffin_lim(small, stft, 0, seed=5)[1])


def test_device_phase_is_the_restated_generator(stft):
    """Y of istft_frames_seeded against istft_frames on theta = 2 pi u from the integer restatement.  Both run the same FFT, so the
    distance is that of the inputs: theta rounded to float32 (half an ulp at 2 pi = 2.4e-7 rad) plus sincosf's ulp or two against the
    kernel's sincospi(2 u) - bound 1e-6 relative L2; a wrong counter gives O(1)"""
    B, F = 2, 64
    mag = torch.from_numpy(_magnitudes(B, F, 93)).to(DEV)
    ws = stft._workspace(mag, "magnitude")
    for seed in (0, 12345, -3, (1 << 40) + 17):
        s = torch.tensor([seed], dtype=torch.int64, device=DEV)
        Y, magT = K.istft_frames_seeded(mag, ws, s, want_magT=True)
        th = torch.from_numpy(FR.device_phase(seed, B, F).astype(np.float32)).to(DEV)
        Yr, magTr = K.istft_frames(mag, th, ws, want_magT=True)
        assert torch.equal(magT, magTr)
        err = R.rel_l2(_np(Y), _np(Yr))
        print(f"seed {seed}: seeded frames vs frames of the restated phase, rel-L2 {err:.3e}")
        assert err < 1e-6


def test_device_phase_is_uniform_on_the_circle(stft):
    """one [2, 513, 64] draw, recovered through STFT.transform of the inverse of mag = 1: the means of cos and sin lie within
    4 / sqrt(n) of 0 (the projection onto consistent spectrograms mixes neighbouring bins and keeps a uniform phase uniform)"""
    mag = torch.ones(2, 513, 64, device=DEV)
    sig = audio.griffin_lim(mag, stft, 0, seed=2024)
    assert torch.isfinite(sig).all() and sig.abs().max() > 0
    _, p = stft.transform(sig)
    assert p.shape == (2, 513, 64)
    n = p.numel()
    c, s = float(torch.cos(p.double()).mean()), float(torch.sin(p.double()).mean())
    print(f"mean cos {c:.3e}, mean sin {s:.3e}, bound {4 / np.sqrt(n):.3e}")
    assert abs(c) < 4 / np.sqrt(n) and abs(s) < 4 / np.sqrt(n)


# ---- what it is for
def test_momentum_32_iterations_converge_below_plain_60_on_the_device(stft):
    mag = R.speechlike_magnitude(200, 8)
    m, a = _dev(mag, R.seeded_angles(mag.shape, 12))

    def conv(sig):
        got, _ = stft.transform(sig)
        return float((got.double() - m.double()).norm() / m.double().norm())
    plain = conv(audio.griffin_lim(m, stft, 60, angles=a))
    fast = conv(audio.griffin_lim(m, stft, 32, angles=a, momentum=MOM))
    print(f"spectral convergence: plain x 60 {plain:.4f}, momentum 0.99 x 32 {fast:.4f}")
    assert fast < plain


def test_inv_mel_spec_passes_momentum_and_seed_through(tmp_path):
    from scipy.io.wavfile import read
    t = audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    mel = torch.from_numpy(R.g19_mel()).to(DEV)
    paths = [str(tmp_path / f"{i}.wav") for i in range(3)]
    audio.inv_mel_spec(mel, paths[0], t, 16, momentum=MOM, seed=3)
    audio.inv_mel_spec(mel, paths[1], t, 16, momentum=MOM, seed=3)
    audio.inv_mel_spec(mel, paths[2], t, 16, momentum=0.0, seed=3)
    w = [read(p)[1] for p in paths]
    assert w[0].shape == (256 * 31,) and np.isfinite(w[0]).all()
    assert np.array_equal(w[0], w[1]) and not np.array_equal(w[0], w[2])
    spec = (torch.exp(mel).t() @ t.mel_basis).t().unsqueeze(0)[:, :, :-1] * 1000.0
    assert np.array_equal(w[0], audio.griffin_lim(spec, t.stft_fn, 16, momentum=MOM, seed=3)[0].cpu().numpy())


def test_abi_refuses_bad_arguments(stft):
    mag = torch.rand(1, 513, 8, device=DEV)
    ws = stft._workspace(mag, "magnitude")
    Y, magT = K.istft_frames(mag, torch.zeros_like(mag), ws, want_magT=True)
    state = K.griffinlim_state(1, 8, DEV)
    for coef in (-0.1, 1.0, float("nan")):
        with pytest.raises(_lib.CttsError):
            K.griffinlim_iter_momentum(Y, magT, state, ws, torch.empty_like(Y), coef, True)
    with pytest.raises(_lib.CttsError):                      # in place: Y_in is read by neighbouring frames
        K.griffinlim_iter_momentum(Y, magT, state, ws, Y, COEF, True)
    with pytest.raises(_lib.CttsError):                      # a state buffer too small for the frames
        K.griffinlim_iter_momentum(Y, magT, state[:100], ws, torch.empty_like(Y), COEF, True)
    Y3 = torch.zeros(1, 3, 1024, device=DEV)
    with pytest.raises(_lib.CttsError):                      # F < 4
        K.griffinlim_iter_momentum(Y3, torch.zeros(1, 3, 513, device=DEV), state, ws, torch.empty_like(Y3), COEF, True)
