"""CPU: the float64 layer model of tests/vocoder_layer_restate.py against torch's own convolutions, and the kernels' index walk - driven by
kernels.vocoder_pack_weight(w, u, planes=False), which is pure torch - against that model, dense and ragged, over the geometry lists
the GPU contract test (tests/test_vocoder_contract_gpu.py) runs.  This pins the packer's layout and vc_geometry's formulas
(csrc/vocoder_common.h) without a GPU; what is left for the GPU is the tile code."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import kernels as K  # noqa: E402
import vocoder_layer_restate as M  # noqa: E402

CH = [(32, 32), (16, 8), (20, 12), (40, 24), (64, 48)]
TS_UP = [1, 2, 37, 127, 128, 129, 300]
CH_CONV = [(1, 1), (3, 5), (8, 8), (16, 8), (20, 36), (33, 31), (80, 100), (36, 130)]
TS_CONV = [1, 2, 63, 128, 129, 200]


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _case(B, T, cin, cout, k, u, g):
    x = _ints((B, T, cin), -4, 4, g)
    w = _ints((cin, cout, k) if u else (cout, cin, k), -2, 2, g)
    Tout = T * u if u else T
    return x, w, _ints((cout,), -4, 4, g), _ints((B, Tout, cout), -4, 4, g), _ints((B, Tout, cout), -4, 4, g)


@pytest.mark.parametrize("k,u", M.KU)
def test_model_equals_conv_transpose1d(k, u):
    g = torch.Generator().manual_seed(k * 131 + u)
    for (cin, cout), T in zip(CH + CH[:2], TS_UP):
        x, w, bias, R, old = _case(2, T, cin, cout, k, u, g)
        a = torch.where(x > 0, x, x * 0.5)                           # slope 0.5 on integers: exact
        conv = F.conv_transpose1d(a.transpose(1, 2), w, None, u, (k - u) // 2).transpose(1, 2)
        want = 2.0 * old + 0.5 * (conv + bias + R)
        wmag = F.conv_transpose1d(a.abs().transpose(1, 2), w.abs(), None, u, (k - u) // 2).transpose(1, 2) + bias.abs() + R.abs()
        out, mag, stored = M.conv_layer(x, w, 1, u, 0.5, bias, R, old, 0.5, 2.0)
        assert out.shape == (2, T * u, cout) and stored.all()
        assert torch.equal(out, want) and torch.equal(mag, wmag), (cin, cout, T)
        out0, _, _ = M.conv_layer(x, w, 1, u, None, None, None, None)                # nothing of the epilogue, no activation
        assert torch.equal(out0, F.conv_transpose1d(x.transpose(1, 2), w, None, u, (k - u) // 2).transpose(1, 2))


@pytest.mark.parametrize("k,dil", M.KD)
def test_model_equals_conv1d(k, dil):
    g = torch.Generator().manual_seed(k * 131 + dil)
    pad = dil * (k - 1) // 2
    for i, (cin, cout) in enumerate(CH_CONV):
        for T in (TS_CONV[i % 6], TS_CONV[(i + 3) % 6]):
            x, w, bias, R, old = _case(2, T, cin, cout, k, 0, g)
            a = torch.where(x > 0, x, x * 0.5)
            conv = F.conv1d(a.transpose(1, 2), w, None, 1, pad, dil).transpose(1, 2)
            out, mag, stored = M.conv_layer(x, w, dil, 0, 0.5, bias, R, old, 0.5, 2.0)
            assert stored.all() and torch.equal(out, 2.0 * old + 0.5 * (conv + bias + R)), (cin, cout, T)
            assert torch.equal(mag, F.conv1d(a.abs().transpose(1, 2), w.abs(), None, 1, pad, dil).transpose(1, 2) + bias.abs() + R.abs())


def test_model_half_operand_and_lengths():
    """half=True rounds the activated operand as the fp16 mode stages it; an utterance is computed from its own rows alone"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 9, 4, generator=g) * 100
    x[0, 0, 0], x[0, 0, 1] = 1e6, -1e7
    a = M.operand(x, 0.1, half=True)
    x32 = torch.where(x > 0, x, x * 0.1)
    assert torch.equal(a, x32.clamp(-65504, 65504).half().double()) and a[0, 0, 0] == 65504.0 and a[0, 0, 1] == -65504.0
    w = torch.randn(4, 5, 6, generator=g)
    lens, len_mul = [2, 0, 9], 3                                     # rows 6, 0, 9 (clamped to T)
    xn = x.clone()
    xn[0, 6:], xn[1] = float("nan"), float("nan")
    out, mag, stored = M.conv_layer(xn, w, 1, 2, 0.1, lens=lens, len_mul=len_mul)
    assert stored.sum(1).tolist() == [12, 0, 18]
    assert torch.equal(out[0, :12], M.conv_layer(x[:1, :6], w, 1, 2, 0.1)[0][0]) and out[0, 12:].isnan().all() and out[1].isnan().all()
    assert torch.equal(out[2], M.conv_layer(x[2:], w, 1, 2, 0.1)[0][0]) and not out[stored].isnan().any()


def _lens_for(T):
    """(lens, len_mul) lists whose products reach 0, 1, the rows next to a 128-row tile edge, T and beyond T"""
    return [([0, 1, 127, 128, 129, T, 9999, -3], 1), ([0, 1, 43, T // 3 + 1, 42], 3)]


@pytest.mark.parametrize("k,u", M.KU)
def test_walk_of_packed_weight_equals_model_transposed(k, u):
    g = torch.Generator().manual_seed(k * 17 + u)
    i = M.KU.index((k, u))
    for cin, cout in (CH[i % 5], CH[(i + 2) % 5]):
        for T in (TS_UP[i % 7], TS_UP[(i + 3) % 7], 128 if i % 2 else 127):
            x, w, *_ = _case(2, T, cin, cout, k, u, g)
            geo = M.geometry(T, k, 1, u)
            assert geo is not None and geo["taps"] == k // u and geo["pad"] == (k - u) // 2
            packed, planes = K.vocoder_pack_weight(w.float(), u, planes=False)
            assert planes is None
            out, count = M.walk(x, packed, cin, cout, **geo)
            want, _, stored = M.conv_layer(x, w, 1, u)
            assert stored.all() and (count == 1).all(), (cin, cout, T, count.min().item(), count.max().item())
            assert torch.equal(out, want), (cin, cout, T)
    cin, cout = CH[(i + 1) % 5]
    T = 140
    for lens, len_mul in _lens_for(T):
        B = len(lens)
        x, w, *_ = _case(B, T, cin, cout, k, u, g)
        for b in range(B):
            x[b, M.rows_of(lens, b, len_mul, T):] = float("nan")
        packed, _ = K.vocoder_pack_weight(w.float(), u, planes=False)
        out, count = M.walk(x, packed, cin, cout, lens=lens, len_mul=len_mul, **M.geometry(T, k, 1, u))
        want, _, stored = M.conv_layer(x, w, 1, u, lens=lens, len_mul=len_mul)
        assert torch.equal(count, stored[:, :, None].expand_as(count).long()), (lens, len_mul)     # stored rows once, the others never
        assert torch.equal(out[stored], want[stored]) and not out.isnan().any()


@pytest.mark.parametrize("k,dil", M.KD)
def test_walk_of_packed_weight_equals_model_conv1d(k, dil):
    g = torch.Generator().manual_seed(k * 17 + dil)
    for i, (cin, cout) in enumerate(CH_CONV):
        T = TS_CONV[(i + k) % 6]
        x, w, *_ = _case(2, T, cin, cout, k, 0, g)
        geo = M.geometry(T, k, dil, 0)
        assert geo["mextra"] == 0 and geo["row_off"] == 0 and (geo["taps"] - 1) * geo["dil"] <= 64
        packed, _ = K.vocoder_pack_weight(w.float(), 0, planes=False)
        out, count = M.walk(x, packed, cin, cout, **geo)
        assert (count == 1).all() and torch.equal(out, M.conv_layer(x, w, dil)[0]), (cin, cout, T)
    cin, cout, T = 20, 36, 140
    for lens, len_mul in _lens_for(T):
        x, w, *_ = _case(len(lens), T, cin, cout, k, 0, g)
        for b in range(len(lens)):
            x[b, M.rows_of(lens, b, len_mul, T):] = float("nan")
        packed, _ = K.vocoder_pack_weight(w.float(), 0, planes=False)
        out, count = M.walk(x, packed, cin, cout, lens=lens, len_mul=len_mul, **M.geometry(T, k, dil, 0))
        want, _, stored = M.conv_layer(x, w, dil, lens=lens, len_mul=len_mul)
        assert torch.equal(count, stored[:, :, None].expand_as(count).long()) and torch.equal(out[stored], want[stored])
        assert not out.isnan().any()


def test_geometry_names_the_paths_and_the_refusals():
    """the path each (k, u) of the list is there for, and what vc_geometry refuses"""
    geo = {ku: M.geometry(100, ku[0], 1, ku[1]) for ku in M.KU}
    for ku in [(2, 2), (3, 3), (8, 8)]:
        assert (geo[ku]["taps"], geo[ku]["pad"], geo[ku]["mextra"], geo[ku]["row_off"]) == (1, 0, 0, 0)
    for ku in [(1, 1), (3, 1), (5, 1)]:
        assert geo[ku]["row_off"] == geo[ku]["pad"] == (ku[0] - 1) // 2 and geo[ku]["mextra"] == 0
    for ku in [(4, 2), (16, 8)]:
        assert (geo[ku]["taps"], geo[ku]["row_off"], geo[ku]["mextra"]) == (2, 0, 1)
    for ku in [(6, 2), (12, 4), (9, 3)]:
        assert (geo[ku]["taps"], geo[ku]["row_off"], geo[ku]["mextra"]) == (3, 1, 0)
    for ku in [(8, 2), (16, 4)]:
        assert (geo[ku]["taps"], geo[ku]["row_off"], geo[ku]["mextra"]) == (4, 1, 1)
    for ku in [(10, 2), (15, 3), (24, 4)]:
        assert geo[ku]["row_off"] == 2
    assert geo[(130, 2)]["taps"] == 65 and geo[(130, 2)]["in_off"] == -64
    assert sum((k - 1) * d == 64 for k, d in M.KD) == 5 and all(M.geometry(9, k, d, 0) for k, d in M.KD)
    for k, d, u in [(3, 33, 0), (67, 1, 0), (4, 1, 0), (132, 2, 2), (5, 1, 2), (6, 1, 3), (7, 1, 2)]:
        assert M.geometry(9, k, d, u) is None, (k, d, u)


def test_conv_post_model_equals_conv1d():
    g = torch.Generator().manual_seed(9)
    for C, k, T in [(1, 1, 1), (8, 3, 3), (31, 7, 40), (33, 31, 12), (80, 7, 300)]:
        x = torch.randn(2, T, C, generator=g)
        w, bias = torch.randn(k, C, generator=g) / (k * C) ** 0.5, torch.randn(1, generator=g)
        a = torch.where(x.double() > 0, x.double(), x.double() * M.slope32(0.01))
        want = F.conv1d(a.transpose(1, 2), w.double().t()[None], bias.double(), 1, (k - 1) // 2)[:, 0]
        pre, mag, wav = M.conv_post(x, w, bias, 0.01)
        assert (pre - want).abs().max().item() <= 1e-13 and torch.equal(wav, torch.tanh(pre)) and (mag >= pre.abs() - 1e-13).all()
        n = max(T // 2, 1)
        xn = x.clone()
        xn[1, n:] = float("nan")
        pre2, _, wav2 = M.conv_post(xn, w, bias, 0.01, lens=[T + 5, n], len_mul=1)
        assert (pre2[0] - pre[0]).abs().max().item() <= 1e-13             # float64 rounding: a batched matmul may sum in another order
        assert torch.equal(wav2[1, :n], M.conv_post(x[1:, :n], w, bias, 0.01)[2][0])
        assert (wav2[1, n:] == 0).all() and pre2[1, n:].isnan().all() and not wav2.isnan().any()
