"""CPU: the surface of the vocoder's fp16 mode (include/ctts.h "fp16 mode", _lib.py, kernels.vocoder_conv_h / vocoder_post_h,
vocoder.Generator called as g(mel, lens, precision)) and the CPU emulation of its arithmetic contract (tests/hifigan_half_emulation.py)
that test_vocoder_half_gpu.py takes its error bars from."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import _lib, vocoder  # noqa: E402
from ctts_amd import kernels as K  # noqa: E402
from ctts_amd.vocoder import AttrDict, Generator  # noqa: E402
import hifigan_restate as R  # noqa: E402
import hifigan_half_emulation as E  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def _g17():
    return R.load_g17(os.path.join(GOLD, "g17_hifigan_small.npz"))


def _header():
    return open(os.path.join(ROOT, "include", "ctts.h")).read()


def test_emulation_without_rounding_is_the_restatement():
    z, h, sd = _g17()
    W = R.fold_state_dict(sd, dtype=torch.float64)
    mel = torch.from_numpy(z["mel"]).double()
    ref = R.generator_forward(W, h, mel)
    for rev in (False, True):
        out = E.generator_forward_half(W, h, mel, acc_dtype=torch.float64, rounding=False, reverse_channels=rev)
        assert out.shape == ref.shape
        assert (out - ref).abs().max().item() <= 1e-12, rev


def test_emulation_rounding_is_fp16_sized_and_order_matters_in_fp32():
    z, h, sd = _g17()
    mel = torch.from_numpy(z["mel"])
    ref = R.generator_forward(R.fold_state_dict(sd, dtype=torch.float64), h, mel.double())
    W32 = R.fold_state_dict(sd, dtype=torch.float32)
    e64 = (E.generator_forward_half(W32, h, mel, acc_dtype=torch.float64) - ref).abs().max().item()
    a = E.generator_forward_half(W32, h, mel, acc_dtype=torch.float32)
    b = E.generator_forward_half(W32, h, mel, acc_dtype=torch.float32, reverse_channels=True)
    ea, eb = (a.double() - ref).abs().max().item(), (b.double() - ref).abs().max().item()
    print(f"g17 fp16 emulation vs float64: acc64 {e64:.3e}, acc32 {ea:.3e}, acc32 reversed {eb:.3e}, wav std {ref.std().item():.3f}")
    for e in (e64, ea, eb):
        assert 1e-6 < e < 5e-2           # far above fp32 noise (the rounding is on), far below the signal


def test_round_half_saturates_and_rounds_to_nearest_even():
    x = torch.tensor([1e6, -1e6, 65519.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25], dtype=torch.float64)
    assert E.round_half(x).tolist() == [65504.0, -65504.0, 65504.0, 1.0, 1.0 + 2.0 ** -9, 0.0, 2.0 ** -23]
    assert torch.equal(E.round_half(x, on=False), x)


def test_default_precision_follows_the_environment(monkeypatch):
    _, h, _ = _g17()
    monkeypatch.delenv(vocoder.PRECISION_ENV, raising=False)
    assert Generator(AttrDict(h)).default_precision == "fp32"
    for v in ("fp32", "fp16"):
        monkeypatch.setenv(vocoder.PRECISION_ENV, v)
        assert Generator(AttrDict(h)).default_precision == v
    monkeypatch.setenv(vocoder.PRECISION_ENV, "bf16")
    with pytest.raises(ValueError, match="precision"):
        Generator(AttrDict(h))


def test_bad_precision_raises_before_any_launch():
    _, h, _ = _g17()
    g = Generator(AttrDict(h))
    for bad in ("half", "bf16", 16, ""):
        with pytest.raises(ValueError, match="precision"):
            g(torch.zeros(1, 80, 4), precision=bad)        # a CPU mel: the value is rejected before the device check
    g.default_precision = "fp64"
    with pytest.raises(ValueError, match="precision"):
        g(torch.zeros(1, 80, 4))
    assert g._call_precision is None                         # a call that raised leaves no precision behind


def test_python_surface_takes_precision():
    ps = inspect.signature(Generator.__call__).parameters
    assert list(ps) == ["self", "x", "lens", "precision"] and ps["lens"].default is None and ps["precision"].default is None
    assert list(inspect.signature(Generator.forward).parameters) == ["self", "x", "lens"]      # what its earlier callers and tests know
    assert list(inspect.signature(vocoder.infer_wavs).parameters) == ["vocoder", "mels", "mel_lens", "max_wav_value"]
    assert list(inspect.signature(Generator.__init__).parameters) == ["self", "h"]


def test_state_dict_keys_and_module_tree_are_unchanged(monkeypatch):
    _, h, sd = _g17()
    monkeypatch.setenv(vocoder.PRECISION_ENV, "fp16")
    g = Generator(AttrDict(h))
    assert sorted(g.state_dict()) == sorted(sd)
    g.load_state_dict(sd)
    g.remove_weight_norm()
    assert sorted(g.state_dict()) == sorted(k.replace("weight_v", "weight") for k in sd if not k.endswith("weight_g"))
    assert [n for n, _ in g.named_children()] == ["conv_pre", "ups", "resblocks", "conv_post"]
    assert not list(g.buffers())


def test_new_symbols_are_declared_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ctts_vocoder_conv_h", "ctts_vocoder_post_h"):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
        assert decl, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name]) == len(decl.group(1).split(","))
    body = re.search(r"typedef struct ctts_vconv_h_desc \{(.*?)\} ctts_vconv_h_desc;", hdr, re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            first, *rest = [p.strip() for p in stmt.split(",")]
            fields += [re.split(r"[\s*]+", first)[-1]] + rest
    assert fields == [n for n, _ in _lib.VconvHDesc._fields_]
    for word in ("v_mfma_f32_32x32x16_f16", "65504", "subnormal", "round to nearest even"):
        assert word in hdr                                   # the arithmetic contract is written where the ABI is
    # the fp32 descriptor is untouched by the new mode
    assert [n for n, _ in _lib.VconvDesc._fields_][-3:] == ["bf16_split", "lens", "len_mul"]


def test_cpu_tensors_raise():
    _, h, sd = _g17()
    g = Generator(AttrDict(h))
    g.load_state_dict(sd)
    with pytest.raises(_lib.CttsError, match="no CPU path"):
        g(torch.zeros(2, 80, 8), precision="fp16")
    with pytest.raises(_lib.CttsError, match="no CPU path"):
        g.default_precision = "fp16"
        vocoder.infer_wavs(g, torch.zeros(2, 80, 8), [8, 3])
    w = torch.zeros(128, 3 * 32, dtype=torch.float16)
    with pytest.raises(_lib.CttsError, match="device"):
        K.vocoder_conv_h(torch.zeros(1, 4, 32, dtype=torch.float16), w, 32, 32, 3)
    with pytest.raises(_lib.CttsError):
        K.vocoder_conv_h(torch.zeros(1, 4, 32, dtype=torch.bfloat16), w, 32, 32, 3)
    with pytest.raises(_lib.CttsError):
        K.vocoder_post_h(torch.zeros(1, 4, 32, dtype=torch.float16), torch.zeros(7, 32), torch.zeros(1))
