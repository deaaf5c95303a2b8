"""CPU: the MelGAN generator's module layout, its float64 restatement and the argument checks of melgan.Generator that need no GPU."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ctts_amd import _lib, melgan  # noqa: E402
import melgan_restate as MR  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def _schema():
    with open(os.path.join(GOLD, "melgan_state_dict_schema.json")) as f:
        return json.load(f)


def test_restatement_matches_the_stock_module_build_in_float64():
    stock = MR.recipe_(MR.stock_generator()).double().eval()
    W = MR.fold_state_dict(stock.state_dict(), dtype=torch.float64)
    mel = torch.randn(2, 80, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        a, b = stock(mel), MR.generator_forward(W, mel)
    assert a.shape == b.shape == (2, 1, 256 * 7)
    assert (a - b).abs().max().item() <= 1e-12
    assert 0.1 <= a.std().item() <= 0.4 and a.abs().max().item() >= 0.5          # the recipe drives the tanh


def test_state_dict_keys_and_shapes_match_the_schema():
    sch = _schema()
    assert sch["entries"] == len(sch["keys"]) == 126 and sch["parameters"] == 4266050
    g = melgan.Generator()
    sd = g.state_dict()
    assert list(sd) == list(sch["keys"])
    assert {k: list(v.shape) for k, v in sd.items()} == sch["keys"]
    assert sum(v.numel() for v in sd.values()) == 4266050
    assert list(MR.stock_generator().state_dict()) == list(sch["keys"])
    for k in ("model.1.bias", "model.1.weight_g", "model.1.weight_v", "model.3.weight_v", "model.4.block.2.weight_g", "model.4.block.4.bias",
              "model.4.shortcut.weight_v", "model.21.shortcut.bias", "model.24.weight_v"):
        assert k in sd, k
    assert MR.flops_per_frame() == 90341376


def test_both_weight_forms_load():
    sd = MR.recipe_state_dict()
    g = melgan.Generator()
    g.load_state_dict(sd)                                                       # weight norm
    W = MR.fold_state_dict(sd, dtype=torch.float32)
    g.remove_weight_norm()
    folded = g.state_dict()
    assert len(folded) == 84 and not any(k.endswith(("weight_g", "weight_v")) for k in folded)
    for p, (w, b) in W.items():
        assert (folded[p + ".weight"] - w).abs().max().item() <= 1e-6 and torch.equal(folded[p + ".bias"], b), p
    g2 = melgan.Generator()
    g2.remove_weight_norm()
    g2.load_state_dict(folded)                                                  # folded
    v = melgan.load_melgan(folded, device="cpu")
    assert isinstance(v, melgan.MelVocoder) and torch.equal(v.mel2wav.state_dict()["model.24.weight"], folded["model.24.weight"])
    v = melgan.load_melgan(sd, device="cpu")
    assert torch.equal(v.mel2wav.state_dict()["model.24.weight_v"], sd["model.24.weight_v"]) and not v.mel2wav.training


def test_cpu_tensor_and_short_mel_raise():
    g = melgan.Generator()
    with pytest.raises(_lib.CttsError, match="device"):
        g(torch.zeros(1, 80, 8))
    with pytest.raises(_lib.CttsError, match="at least 4 frames"):
        g(torch.zeros(1, 80, 3))
    with pytest.raises(_lib.CttsError, match="device"):                         # T = 4 passes the length check: what is left is the device
        g(torch.zeros(1, 80, 4))
    with pytest.raises(_lib.CttsError, match=r"expected mel \[B, 80, T\]"):
        g(torch.zeros(1, 79, 8))


def test_kernel_wrappers_reject_bad_modes_before_any_launch():
    from ctts_amd import kernels as K
    with pytest.raises(_lib.CttsError, match="pad_mode"):
        K.vocoder_conv(torch.zeros(1, 8, 32), None, None, 32, 32, 3, bf16_split=0, pad_mode="edge")
    with pytest.raises(_lib.CttsError, match="Conv1d only"):
        K.vocoder_conv(torch.zeros(1, 8, 32), None, None, 32, 32, 4, transposed_u=2, bf16_split=0, pad_mode="reflect")
    with pytest.raises(_lib.CttsError, match="reflection needs T"):
        K.vocoder_conv(torch.zeros(1, 9, 32), None, None, 32, 32, 3, 9, bf16_split=0, pad_mode="reflect")
    with pytest.raises(_lib.CttsError, match="1x1 Conv1d only"):
        K.vocoder_conv(torch.zeros(1, 8, 32), None, None, 32, 32, 3, bf16_split=0, x2=torch.zeros(1, 8, 32))
    w, pl = K.vocoder_pack_weight(torch.ones(40, 33, 1), planes=False, weight2=2 * torch.ones(40, 70, 1))
    assert pl is None and tuple(w.shape) == (128, 64 + 96)
    assert w[:40, :33].eq(1).all() and w[:40, 33:64].eq(0).all() and w[:40, 64:134].eq(2).all() and w[:40, 134:].eq(0).all() and w[40:].eq(0).all()
    with pytest.raises(_lib.CttsError, match="two-operand"):
        K.vocoder_pack_weight(torch.ones(40, 33, 3), planes=False, weight2=torch.ones(40, 70, 1))
