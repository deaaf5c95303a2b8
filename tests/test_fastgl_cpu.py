"""CPU: fast Griffin-Lim (momentum) and the device initial phase - the float64 oracle (tests/fastgl_restate.py), the C ABI's new entry
points and the argument checks of audio.griffin_lim.  The kernels themselves are tested in test_fastgl_gpu.py."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import _lib, audio  # noqa: E402
import fastgl_restate as FR  # noqa: E402
import griffinlim_restate as R  # noqa: E402

NEW_SYMBOLS = ["ctts_griffinlim_iter_momentum", "ctts_griffinlim_state_floats", "ctts_istft_frames_seeded"]
# (magnitude, seed of the initial phase): the three inputs of the convergence table in DESIGN.md section 10
INPUTS = {"g19": (R.g19_gl_magnitude, R.GL_SEED), "speech64": (lambda: R.speechlike_magnitude(64, 7), 11),
          "speech200": (lambda: R.speechlike_magnitude(200, 8), 12)}


@pytest.mark.parametrize("name", ["g19", "speech64"])
def test_momentum_zero_is_the_plain_restatement(name):
    make, seed = INPUTS[name]
    mag = make()
    ang = R.seeded_angles(mag.shape, seed)
    for n in (0, 1, 8):
        assert R.rel_l2(FR.griffin_lim(mag, ang, n, momentum=0.0), R.griffin_lim(mag, ang, n)) < 1e-12


def test_first_iteration_has_no_momentum_term():
    mag = R.g19_gl_magnitude()
    ang = R.seeded_angles(mag.shape, R.GL_SEED)
    assert R.rel_l2(FR.griffin_lim(mag, ang, 1, momentum=0.99), R.griffin_lim(mag, ang, 1)) < 1e-12
    assert R.rel_l2(FR.griffin_lim(mag, ang, 2, momentum=0.99), R.griffin_lim(mag, ang, 2)) > 1e-3


@pytest.mark.parametrize("name", list(INPUTS))
def test_momentum_halves_the_iterations_to_equal_convergence(name):
    """spectral convergence || |STFT(x)| - mag || / || mag || from the same seeded start: momentum 0.99 after 32 iterations is below
    the plain loop after 60, and after 16 below the plain loop after 32"""
    make, seed = INPUTS[name]
    mag = make()
    ang = R.seeded_angles(mag.shape, seed)
    plain = {n: FR.spectral_convergence(R.griffin_lim(mag, ang, n), mag) for n in (32, 60)}
    fast = {n: FR.spectral_convergence(FR.griffin_lim(mag, ang, n, momentum=0.99), mag) for n in (16, 32)}
    print(name, "plain", plain, "momentum 0.99", fast)
    assert fast[32] < plain[60]
    assert fast[16] < plain[32]


def test_zero_magnitude_rule_is_the_kernels():
    """a bin whose A is exactly 0 becomes (magnitude, 0): np.angle(0) = 0, no 1e-16 regulariser"""
    assert np.angle(0j) == 0.0
    mag = np.zeros((1, 513, 8))
    out = FR.griffin_lim(mag, np.zeros_like(mag), 3)
    assert np.isfinite(out).all() and not out.any()


def test_device_phase_restatement_is_a_function_of_seed_b_k_f_alone():
    u = FR.device_phase_u(7, 1, 64)
    assert u.shape == (513, 64) and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u[:, :40], FR.device_phase_u(7, 1, 40))            # a longer batch appends frames, changes none
    assert np.array_equal(FR.device_phase(7, 3, 16)[1], 2 * np.pi * FR.device_phase_u(7, 1, 16))
    assert not np.array_equal(u, FR.device_phase_u(8, 1, 64)) and not np.array_equal(u, FR.device_phase_u(7, 2, 64))
    assert np.array_equal(FR.device_phase_u(-1, 0, 4), FR.device_phase_u(2 ** 64 - 1, 0, 4))
    th = FR.device_phase(123, 2, 64)
    n = th.size
    assert abs(np.cos(th).mean()) < 4 / np.sqrt(n) and abs(np.sin(th).mean()) < 4 / np.sqrt(n)
    assert abs(u.mean() - 0.5) < 4 * np.sqrt(1 / 12.0 / u.size)


def test_new_symbols_declared_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, "include", "ctts.h")).read()
    declared = set(re.findall(r"\b(ctts_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    bound = _lib.load()
    for name in ("ctts_griffinlim_iter_momentum", "ctts_istft_frames_seeded"):
        assert getattr(bound, name).argtypes == _lib._SIGNATURES[name]
    # one slot per frame, at least the 513 complex bins; 0 for an empty batch
    assert bound.ctts_griffinlim_state_floats(3, 7) >= 3 * 7 * 2 * 513
    assert bound.ctts_griffinlim_state_floats(3, 7) == 21 * bound.ctts_griffinlim_state_floats(1, 1)
    assert bound.ctts_griffinlim_state_floats(0, 7) == 0
    # the ABI only grows: the plain entry points keep their argument lists
    assert re.search(r"int ctts_griffinlim_iter\(const float\* Y_in, const float\* magT, const int32_t\* frames, const float\* workspace, "
                     r"float\* Y_out, int B, int F,\s+int n_fft, int hop, void\* stream\);", hdr)
    assert len(_lib._SIGNATURES["ctts_griffinlim_iter"]) == 10 and len(_lib._SIGNATURES["ctts_istft_frames"]) == 14


def test_python_surface():
    from ctts_amd import kernels as K
    for name in ("griffinlim_iter_momentum", "griffinlim_state", "istft_frames_seeded"):
        assert callable(getattr(K, name))
    p = inspect.signature(audio.griffin_lim).parameters
    assert list(p) == ["magnitudes", "stft_fn", "n_iters", "angles", "lens", "momentum", "seed"]
    assert p["n_iters"].default == 30 and p["momentum"].default == 0.0 and p["seed"].default is None
    p = inspect.signature(audio.inv_mel_spec).parameters
    assert list(p) == ["mel", "out_filename", "_stft", "griffin_iters", "momentum", "seed"]
    assert p["griffin_iters"].default == 60 and p["momentum"].default == 0.0 and p["seed"].default is None


def test_argument_errors_come_before_any_device_work():
    """every check below runs on CPU tensors: the ValueErrors are raised ahead of the 'device tensor' RuntimeError"""
    s = audio.STFT(1024, 256, 1024)
    mag = torch.zeros(1, 513, 8)
    for m in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="momentum"):
            audio.griffin_lim(mag, s, 2, momentum=m)
    with pytest.raises(ValueError, match="angles"):
        audio.griffin_lim(mag, s, 2, angles=torch.zeros(1, 513, 8), seed=3)
    with pytest.raises(ValueError, match="angles"):
        audio.griffin_lim(mag, s, 2, angles=torch.zeros(1, 513, 8), seed=torch.tensor([3]))
    for bad in (1.5, "7", True, torch.tensor([1, 2]), torch.tensor([3], dtype=torch.int32), torch.tensor([3.0])):
        with pytest.raises(ValueError, match="seed"):
            audio.griffin_lim(mag, s, 2, seed=bad)
    # valid arguments reach the device check, as before
    for kw in ({"momentum": 0.99}, {"seed": 5}, {"momentum": 0.5, "seed": torch.tensor([5])}, {"momentum": 0.0}):
        with pytest.raises(RuntimeError, match="device"):
            audio.griffin_lim(mag, s, 2, **kw)
