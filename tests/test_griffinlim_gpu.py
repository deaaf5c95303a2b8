"""GPU: the Griffin-Lim vocoder's kernels (csrc/griffinlim.hip through ctts_amd.audio STFT / griffin_lim / inv_mel_spec) against the
reference fixture tests/golden/g19_griffinlim.npz and the float64 restatement tests/griffinlim_restate.py.

Tolerances are stated against the reference's OWN float32 error: g19 records how far its float32 Griffin-Lim drifts from a float64 copy
of the same module after n iterations (drift_rel_l2_n, 4e-7 ... 8e-6); the native result must stay within DRIFT_X times that distance
of both the fixture and float64."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import _lib, audio, kernels as K  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402
import griffinlim_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DRIFT_X = 4.0
G19 = np.load(os.path.join(ROOT, "tests", "golden", "g19_griffinlim.npz"))


@pytest.fixture(scope="module")
def stft():
    return audio.STFT(1024, 256, 1024)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _magnitudes(B, F, seed):
    rs = np.random.RandomState(seed)
    env = 2.0 / (1.0 + np.arange(513) / 30.0)
    return (rs.rand(B, 513, F) * env[None, :, None]).astype(np.float32)


def test_transform_matches_fixture_and_fp64(stft):
    x = R.g19_signal()
    mag, phase = stft.transform(torch.from_numpy(x).to(DEV))
    assert mag.shape == phase.shape == (1, 513, 16) and mag.dtype == torch.float32
    m64, p64 = R.transform(x)
    m, p = _np(mag), _np(phase)
    for f in (np.cos, np.sin):     # rectangular parts: the raw angle is ill-conditioned where |X| ~ 0
        assert R.rel_l2(m * f(p), G19["tr_mag"] * f(G19["tr_phase"])) < 3e-6
        assert R.rel_l2(m * f(p), m64 * f(p64)) < 3e-6
    assert R.rel_l2(m, m64) < 3e-6


def test_transform_ragged_equals_single_calls(stft):
    rs = np.random.RandomState(3)
    lens = [4000, 513, 2817]
    x = np.zeros((3, 4000), dtype=np.float32)
    for i, n in enumerate(lens):
        x[i, :n] = rs.uniform(-0.5, 0.5, n)
    x[1, 513:] = 0.9            # padding must not leak into a shorter utterance
    mag, phase = stft.transform(torch.from_numpy(x).to(DEV), lens=lens)
    for i, n in enumerate(lens):
        m1, p1 = stft.transform(torch.from_numpy(x[i:i + 1, :n]).to(DEV))
        F = 1 + n // 256
        assert torch.equal(mag[i:i + 1, :, :F], m1) and torch.equal(phase[i:i + 1, :, :F], p1)
        assert not mag[i, :, F:].any()


@pytest.mark.parametrize("F", [2, 3, 4, 5, 87, 1024])
def test_inverse_matches_fixture_and_fp64(stft, F):
    m, p = R.g19_inverse_inputs(F)
    out = stft.inverse(torch.from_numpy(m).to(DEV), torch.from_numpy(p).to(DEV))
    assert out.shape == (1, 1, 256 * (F - 1)) and out.dtype == torch.float32
    o = _np(out)
    ref = R.inverse(m, p)
    assert R.rel_l2(o, ref) < 3e-6
    # the window-sum edges (fewer than 4 overlapping frames) on their own
    for sl in (slice(0, 768), slice(-768, None)):
        assert R.rel_l2(o[..., sl], ref[..., sl]) < 5e-6
    if f"inv_F{F}" in G19:
        assert R.rel_l2(o, G19[f"inv_F{F}"]) < 3e-6


@pytest.mark.parametrize("n", R.GL_ITERS)
def test_griffin_lim_matches_fixture_and_fp64(stft, n):
    mag = R.g19_gl_magnitude()
    ang = R.seeded_angles(mag.shape, R.GL_SEED)
    out = audio.griffin_lim(torch.from_numpy(mag).to(DEV), stft, n, angles=torch.from_numpy(ang).to(DEV))
    assert out.shape == (1, 256 * 31)
    tol = DRIFT_X * float(G19[f"drift_rel_l2_{n}"])
    assert R.rel_l2(_np(out), G19[f"gl_{n}"]) < tol
    assert R.rel_l2(_np(out), R.griffin_lim(mag, ang, n)) < tol
    # angles=None draws from numpy's global generator exactly like the reference
    np.random.seed(R.GL_SEED)
    out2 = audio.griffin_lim(torch.from_numpy(mag).to(DEV), stft, n)
    assert torch.equal(out, out2)


def test_griffin_lim_canonical_ragged_batch_vs_fp64(stft):
    """the canonical mel lengths (84 ... 1024 frames) in one ragged batch, 60 iterations, against float64 per utterance.  Griffin-Lim's
    conditioning depends on the input and grows with the length (rounding of ANY float32 implementation is amplified by the iteration):
    the reference algorithm itself at float32 (StockSTFT: its dense-basis GEMMs) lands 3e-5 ... 4e-4 from float64 at these lengths, and
    which utterances amplify the most differs between two float32 implementations.  Bounds: across the batch the native result is at
    least as accurate as that float32 reference (median), and every utterance stays within DRIFT_X x the worst float32-reference error
    of the batch (measured: native median 2e-5, two utterances at 5.5e-4; the float32 reference median 5e-5, worst 4e-4)"""
    lens = [min(int(v), 1024) for v in make_batch(seed=1234)["mel_lens"]]
    B, Fmax = len(lens), max(lens)
    mag = np.zeros((B, 513, Fmax), dtype=np.float32)
    for b, F in enumerate(lens):
        mag[b, :, :F] = R.speechlike_magnitude(F, 100 + b)[0]
    mag[:, :, -1] += 0.5                                   # padding frames carry data: it must not leak
    ang = R.seeded_angles(mag.shape, 22)
    out = audio.griffin_lim(torch.from_numpy(mag).to(DEV), stft, 60, angles=torch.from_numpy(ang).to(DEV), lens=lens)
    assert out.shape == (B, 256 * (Fmax - 1))
    o = _np(out)
    stock = R.StockSTFT(DEV)
    owns = []
    with torch.no_grad():
        for b, F in enumerate(lens):
            m, a = (torch.from_numpy(v[b:b + 1, :, :F]).to(DEV) for v in (mag, ang))
            owns.append(_np(stock.griffin_lim(m, a, 60)))
    res = []
    for b, F in enumerate(lens):
        L = 256 * (F - 1)
        m, a = mag[b:b + 1, :, :F], ang[b:b + 1, :, :F]
        ref = R.griffin_lim(m, a, 60)
        res.append((b, F, R.rel_l2(o[b:b + 1, :L], ref), R.rel_l2(owns[b], ref)))
        assert not o[b, L:].any()
    print("(b, F, native rel-L2, stock float32 rel-L2) vs float64:", res)
    errs, owns_ = np.array([r[2] for r in res]), np.array([r[3] for r in res])
    assert np.median(errs) <= np.median(owns_)
    assert errs.max() < DRIFT_X * owns_.max()


def test_ragged_batch_equals_per_utterance_calls_bitwise(stft):
    lens = [37, 4, 90, 64]
    B, Fmax = len(lens), max(lens)
    mag = torch.from_numpy(_magnitudes(B, Fmax, 31)).to(DEV)
    ang = torch.from_numpy(R.seeded_angles((B, 513, Fmax), 32)).to(DEV)
    out = audio.griffin_lim(mag, stft, 8, angles=ang, lens=lens)
    inv = stft.inverse(mag, ang, lens=lens)
    for b, F in enumerate(lens):
        L = 256 * (F - 1)
        one = audio.griffin_lim(mag[b:b + 1, :, :F], stft, 8, angles=ang[b:b + 1, :, :F])
        assert torch.equal(out[b:b + 1, :L], one), b
        assert torch.equal(inv[b:b + 1, :, :L], stft.inverse(mag[b:b + 1, :, :F], ang[b:b + 1, :, :F])), b


def test_two_runs_and_graph_replay_are_bit_identical(stft):
    lens = [300, 128, 211]
    B, Fmax = len(lens), max(lens)
    mag = torch.from_numpy(_magnitudes(B, Fmax, 41)).to(DEV)
    ang = torch.from_numpy(R.seeded_angles((B, 513, Fmax), 42)).to(DEV)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    eager = audio.griffin_lim(mag, stft, 60, angles=ang, lens=lens_d)
    again = audio.griffin_lim(mag, stft, 60, angles=ang, lens=lens_d)
    assert torch.equal(eager, again)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        audio.griffin_lim(mag, stft, 60, angles=ang, lens=lens_d)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = audio.griffin_lim(mag, stft, 60, angles=ang, lens=lens_d)
    for _ in range(2):
        captured.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)


def _read_wav(path):
    from scipy.io.wavfile import read
    sr, wav = read(path)
    assert sr == 22050 and wav.dtype == np.float32
    return wav


def test_inv_mel_spec_writes_the_fixture_waveform(tmp_path):
    t = audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    path = str(tmp_path / "g19.wav")
    np.random.seed(R.INVMEL_SEED)
    audio.inv_mel_spec(torch.from_numpy(R.g19_mel()).to(DEV), path, t, 60)
    wav = _read_wav(path)
    assert wav.shape == G19["invmel_wav"].shape == (256 * 31,)
    assert R.rel_l2(wav, G19["invmel_wav"]) < DRIFT_X * float(G19["drift_rel_l2_60"]) + 2e-6


def test_inv_mel_spec_reference_style_call_through_dropin(tmp_path):
    """PYTHONPATH=dropin:repo, the reference's own call shape: audio.tools.inv_mel_spec(mel, path, audio.stft.TacotronSTFT(...))"""
    path = str(tmp_path / "x.wav")
    code = textwrap.dedent(f"""
        import sys
        import numpy as np, torch
        sys.path.insert(0, {os.path.join(ROOT, "tests")!r})
        import audio
        import griffinlim_restate as R
        stft = audio.stft.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
        np.random.seed(R.INVMEL_SEED)
        audio.tools.inv_mel_spec(torch.from_numpy(R.g19_mel()).cuda(), {path!r}, stft)
        print("ok")
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr
    assert R.rel_l2(_read_wav(path), G19["invmel_wav"]) < DRIFT_X * float(G19["drift_rel_l2_60"]) + 2e-6


def test_too_few_frames_and_unsupported_sizes_raise(stft):
    mag = torch.rand(1, 513, 3, device=DEV)
    with pytest.raises(ValueError):                         # Griffin-Lim's transform needs more than n_fft/2 samples: F >= 4
        audio.griffin_lim(mag, stft, 2)
    with pytest.raises(ValueError):
        stft.inverse(mag[:, :, :1], mag[:, :, :1])          # the inverse needs F >= 2
    with pytest.raises(ValueError):
        audio.griffin_lim(torch.rand(2, 513, 8, device=DEV), stft, 2, lens=[8, 3])
    with pytest.raises(ValueError):                         # a device lens tensor must hold one length per utterance
        audio.griffin_lim(torch.rand(2, 513, 8, device=DEV), stft, 2, lens=torch.tensor([8], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        stft.transform(torch.zeros(1, 512, device=DEV))
    ws = stft._workspace(mag, "magnitude")
    Y = torch.zeros(1, 3, 1024, device=DEV)
    magT = torch.zeros(1, 3, 513, device=DEV)
    with pytest.raises(_lib.CttsError):                     # the C ABI refuses it as well
        K.griffinlim_iter(Y, magT, ws, torch.empty_like(Y))
    for args in [(2048, 512, 2048), (1024, 200, 800), (1024, 256, 1024, "hamming")]:
        with pytest.raises(NotImplementedError):
            audio.STFT(*args).transform(torch.zeros(1, 4000, device=DEV))
        with pytest.raises(NotImplementedError):
            audio.griffin_lim(torch.rand(1, 513, 8, device=DEV), audio.STFT(*args), 2)
    t = audio.TacotronSTFT(2048, 512, 2048, 80, 22050, 0, 8000).to(DEV)
    with pytest.raises(NotImplementedError):
        audio.inv_mel_spec(torch.zeros(80, 9, device=DEV), "/nonexistent/x.wav", t, 2)


def test_workspace_is_built_when_moved_so_a_first_call_can_be_captured():
    mag = torch.from_numpy(_magnitudes(1, 40, 51)).to(DEV)
    ang = torch.from_numpy(R.seeded_angles((1, 513, 40), 52)).to(DEV)
    eager = audio.griffin_lim(mag, audio.STFT(1024, 256, 1024), 5, angles=ang)
    s = audio.STFT(1024, 256, 1024).to(DEV)
    assert s._ws is not None                                # built by .to(), outside any capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # the first call of this STFT is the captured one
        captured = audio.griffin_lim(mag, s, 5, angles=ang)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
