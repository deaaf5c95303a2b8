"""CPU: the resampling feature's surface - C ABI names, public Python names, the host-side filter design and the refusals that must
happen before anything is launched.  (Numbers: tests/test_resample_restate_cpu.py on the host, tests/test_resample_gpu.py on the device.)"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ctts_amd
from ctts_amd import _lib, kernels as K, preprocess as PP, resample as RS
from ctts_amd._lib import CttsError
from tests import resample_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ctts_resample", "ctts_resample_tile", "ctts_peak_normalize")


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ctts.h")).read()
    declared = set(re.findall(r"\b(ctts_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGNATURES, name
    assert "resample.hip" in open(os.path.join(ROOT, "comprehensive-transformer-tts_amd", "csrc", "build.sh")).read()


def test_public_names():
    assert inspect.ismodule(ctts_amd.resample) and ctts_amd.resample is RS
    for name in ("resample", "resample_filter", "peak_normalize", "polyphase_bank", "PRESETS"):
        assert hasattr(RS, name), name
    assert ctts_amd.resample_filter is RS.resample_filter and ctts_amd.peak_normalize is RS.peak_normalize
    for name in ("resample", "peak_normalize", "resample_tile"):
        assert callable(getattr(K, name)), name
    assert RS.PRESETS["kaiser_best"] == {"zeros": 64, "beta": 14.769656459379492, "rolloff": 0.9475937167399596}
    assert RS.PRESETS["kaiser_fast"] == {"zeros": 16, "beta": 8.555504641634386, "rolloff": 0.85}
    for f in (RS.resample, RS.resample_filter):
        assert "UNPINNED" in RS.__doc__ and f.__doc__


@pytest.mark.parametrize("a,b,want", [(48000, 22050, (147, 320)), (44100, 22050, (1, 2)), (22050, 16000, (320, 441)), (22050, 48000, (320, 147)),
                                      (16000, 22050, (441, 320)), (24000, 22050, (147, 160)), (22050, 44100, (2, 1)), (22050, 24000, (160, 147))])
def test_resample_filter_reduces_the_rates_and_matches_the_restatement(a, b, want):
    for quality, (zeros, beta, rolloff) in R.PRESETS.items():
        L, M, h = RS.resample_filter(a, b, quality)
        assert (L, M) == want and h.dtype == np.float64 and len(h) == 2 * zeros * max(L, M) + 1
        assert np.array_equal(h, R.design(a, b, zeros, beta, rolloff)[3])
    L, M, h = RS.resample_filter(a, b, "kaiser_fast", zeros=4, beta=5.0, rolloff=0.9)
    assert np.array_equal(h, R.design(a, b, 4, 5.0, 0.9)[3])
    bank = RS.polyphase_bank(h, L)
    T = bank.shape[1]
    assert bank.dtype == np.float32 and bank.shape[0] == L and T % K.RESAMPLE_TAP_GRANULE == 0 and T == RS.phase_taps(L, (len(h) - 1) // 2)
    assert 0 <= T - -(-len(h) // L) < K.RESAMPLE_TAP_GRANULE
    assert np.array_equal(bank, R.bank(h, L, T))                             # bank[r][j] == h32[r + j L], zero beyond the end


def test_equal_rates_need_no_filter():
    L, M, h = RS.resample_filter(22050, 22050)
    assert (L, M) == (1, 1) and h.tolist() == [1.0]
    assert RS.resample_filter(48000, 48000, "kaiser_fast")[:2] == (1, 1)


def test_tile_length_is_a_multiple_of_L_and_depends_on_the_filter_only():
    for a, b, zeros in [(48000, 22050, 64), (48000, 22050, 16), (22050, 48000, 64), (2, 1, 4), (1, 2, 64), (441, 320, 64), (1024, 1023, 8)]:
        L, M, h = RS.resample_filter(a, b, zeros=zeros)
        half = (len(h) - 1) // 2
        tile = K.resample_tile(L, M, RS.phase_taps(L, half), half)
        assert tile > 0 and tile % L == 0, (a, b, zeros, tile)
    assert K.resample_tile(1, 1, 8, 0) == 0 and K.resample_tile(2000, 1, 8, 0) == 0 and K.resample_tile(2, 1, 12, 0) == 0


def test_domain_refusals_on_the_host():
    with pytest.raises(ValueError, match="1024"):
        RS.resample_filter(48000, 22051)                                     # coprime: 22051 / 48000
    with pytest.raises(ValueError, match="1024"):
        RS.resample_filter(1025, 1)
    with pytest.raises(ValueError, match="taps per phase"):
        RS.resample_filter(1024, 1)                                          # L = 1: 2 * 64 * 1024 + 1 taps in one phase
    for zeros in (0, 65, 2.5):
        with pytest.raises(ValueError, match="zeros"):
            RS.resample_filter(48000, 22050, zeros=zeros)
    with pytest.raises(ValueError):
        RS.resample_filter(48000, 22050, rolloff=1.5)
    with pytest.raises(ValueError):
        RS.resample_filter(48000, 22050, "sinc_best")
    with pytest.raises(ValueError):
        RS.resample_filter(0, 22050)
    with pytest.raises(ValueError):
        RS.resample_filter(44100.5, 22050)
    with pytest.raises(TypeError):
        RS.resample_filter(48000, 22050, window="hann")


def test_cpu_tensors_raise_without_a_device():
    x = torch.zeros(2, 100)
    with pytest.raises(CttsError, match="no CPU fallback"):
        RS.resample(x, [100, 50], 48000, 22050)
    with pytest.raises(CttsError, match="no CPU fallback"):
        RS.peak_normalize(x, [100, 50])
    with pytest.raises(CttsError):
        K.resample(x, torch.zeros(2, dtype=torch.int32), None, 1, 1, 0)
    with pytest.raises(CttsError):
        K.peak_normalize(x, torch.zeros(2, dtype=torch.int32))


def test_process_batch_keeps_its_signature():
    sig = inspect.signature(PP.process_batch)
    names = list(sig.parameters)
    assert names[:5] == ["wavs", "n_phones", "stft", "preprocess_config", "spans"]
    assert names[5:] == ["source_rate", "resample_quality"]
    assert sig.parameters["spans"].default is None and sig.parameters["source_rate"].default is None
    assert sig.parameters["resample_quality"].default == "kaiser_best"
