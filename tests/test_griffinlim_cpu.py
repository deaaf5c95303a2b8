"""CPU: the Griffin-Lim vocoder's oracle, C ABI, module surface and drop-in (comprehensive-transformer-tts_amd/audio.py STFT /
griffin_lim / inv_mel_spec, csrc/griffinlim.hip, dropin/audio/).  The kernels themselves are tested in test_griffinlim_gpu.py."""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402
from ctts_amd import _lib, audio  # noqa: E402
import griffinlim_restate as R  # noqa: E402

G19 = os.path.join(ROOT, "tests", "golden", "g19_griffinlim.npz")
NEW_SYMBOLS = ["ctts_griffinlim_workspace_bytes", "ctts_griffinlim_prepare", "ctts_stft_transform", "ctts_istft_frames",
               "ctts_griffinlim_iter", "ctts_istft_ola"]


@pytest.fixture(scope="module")
def g19():
    return np.load(G19)


def test_restatement_matches_reference_transform(g19):
    mag, phase = R.transform(R.g19_signal())
    # compare the rectangular parts: the angle is ill-conditioned where |X| ~ 0
    for f in (np.cos, np.sin):
        assert R.rel_l2(mag * f(phase), g19["tr_mag"] * f(g19["tr_phase"])) < 2e-6
    assert R.rel_l2(mag, g19["tr_mag"]) < 2e-6


@pytest.mark.parametrize("F", R.INV_FRAMES)
def test_restatement_matches_reference_inverse(g19, F):
    m, p = R.g19_inverse_inputs(F)
    out = R.inverse(m, p)
    assert out.shape == g19[f"inv_F{F}"].shape == (1, 1, 256 * (F - 1))
    assert R.rel_l2(out, g19[f"inv_F{F}"]) < 2e-6


@pytest.mark.parametrize("n", R.GL_ITERS)
def test_restatement_matches_reference_griffin_lim(g19, n):
    mag = R.g19_gl_magnitude()
    out = R.griffin_lim(mag, R.seeded_angles(mag.shape, R.GL_SEED), n)
    # the reference's own float32 run drifts from float64 by drift_rel_l2_n; the restatement sits at that distance from it
    assert R.rel_l2(out, g19[f"gl_{n}"]) < 3 * float(g19[f"drift_rel_l2_{n}"]) + 1e-6


def test_window_sumsquare_matches_restatement():
    w = audio.window_sumsquare("hann", 7, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32)
    assert w.dtype == np.float32 and w.shape == (1024 + 6 * 256,)
    np.testing.assert_allclose(w, R.window_sumsquare(7), rtol=1e-6, atol=1e-7)


def test_window_sumsquare_general_sizes():
    # hop not dividing n_fft, window shorter than n_fft (centred), one frame: sum of shifted squared windows
    from scipy.signal import get_window
    w2 = np.zeros(1024)
    w2[112:912] = get_window("hann", 800, fftbins=True) ** 2
    for n_frames in (1, 6):
        want = np.zeros(1024 + 200 * (n_frames - 1))
        for f in range(n_frames):
            want[200 * f:200 * f + 1024] += w2
        got = audio.window_sumsquare("hann", n_frames, hop_length=200, win_length=800, n_fft=1024)
        assert got.dtype == np.float32
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)


def test_dynamic_range_round_trip():
    x = torch.tensor([1e-7, 1e-5, 0.5, 3.0])
    c = audio.dynamic_range_compression(x)
    assert torch.allclose(c, torch.log(torch.clamp(x, min=1e-5)))
    assert torch.allclose(audio.dynamic_range_decompression(c)[1:], x[1:])


def test_new_symbols_declared_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, "include", "ctts.h")).read()
    declared = set(re.findall(r"\b(ctts_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    bound = _lib.load()
    for name in NEW_SYMBOLS[1:]:
        assert getattr(bound, name).argtypes == _lib._SIGNATURES[name]
    assert bound.ctts_griffinlim_workspace_bytes(1024, 256) > 0


def test_tacotron_stft_state_dict_unchanged_and_gains_the_reference_members():
    t = audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    assert list(t.state_dict().keys()) == ["mel_basis"]
    assert isinstance(t.stft_fn, audio.STFT)
    x = torch.rand(2, 513, 5) + 0.1
    assert torch.allclose(t.spectral_de_normalize(t.spectral_normalize(x)), x)
    # other FFT sizes still build; only the Griffin-Lim path refuses them
    t2 = audio.TacotronSTFT(2048, 300, 1200, 80, 22050, 0, 8000)
    assert list(t2.state_dict().keys()) == ["mel_basis"]
    with pytest.raises(NotImplementedError):
        t2.stft_fn.transform(torch.zeros(1, 4000))


def test_cpu_tensors_raise():
    s = audio.STFT(1024, 256, 1024)
    with pytest.raises(RuntimeError, match="device"):
        s.transform(torch.zeros(1, 4000))
    with pytest.raises(RuntimeError, match="device"):
        s.inverse(torch.zeros(1, 513, 8), torch.zeros(1, 513, 8))
    with pytest.raises(RuntimeError, match="device"):
        audio.griffin_lim(torch.zeros(1, 513, 8), s, 2)
    t = audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    with pytest.raises(RuntimeError, match="device"):
        audio.inv_mel_spec(torch.zeros(80, 9), "/nonexistent/x.wav", t, 2)


def test_dropin_resolves_the_griffin_lim_names_to_ctts_amd():
    code = textwrap.dedent("""
        import audio
        import audio.stft, audio.audio_processing, audio.tools
        import ctts_amd.audio as A
        assert audio.stft.STFT is A.STFT and audio.stft.TacotronSTFT is A.TacotronSTFT
        assert audio.audio_processing.griffin_lim is A.griffin_lim
        assert audio.audio_processing.window_sumsquare is A.window_sumsquare
        assert audio.audio_processing.dynamic_range_compression is A.dynamic_range_compression
        assert audio.audio_processing.dynamic_range_decompression is A.dynamic_range_decompression
        assert audio.tools.inv_mel_spec is A.inv_mel_spec and audio.tools.get_mel_from_wav is A.get_mel_from_wav
        print("ok")
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
