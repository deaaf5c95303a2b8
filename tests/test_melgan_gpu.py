"""GPU: the MelGAN kernels (reflect-padded conv, two-operand 1x1 tail, reflecting conv_post: csrc/vocoder.hip) and the native
melgan.Generator against float64.  Both arithmetics: the exact three-way bf16 split (default) and exact fp32 MFMA."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ctts_amd import _lib, kernels as K, melgan  # noqa: E402
import melgan_restate as MR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ULP = 2.0 ** -23
NAN = float("nan")


@pytest.fixture(params=[1, 0], ids=["split", "fp32"])
def arith(request):
    prev = K.gemm_bf16_split_enable(request.param)
    yield request.param
    K.gemm_bf16_split_enable(prev)


def lrelu64(x, slope):
    x = x.double()
    return x if slope is None else torch.where(x > 0, x, x * slope)


def reflect_conv_ref64(x, w, bias, d, slope):
    """float64 on the device: x [T, Cin] of ONE utterance, w [Cout, Cin, k] -> [T, Cout] (F.pad reflect + F.conv1d)"""
    pad = d * (w.shape[2] - 1) // 2
    xp = F.pad(lrelu64(x, slope).t()[None], (pad, pad), mode="reflect")
    return F.conv1d(xp, w.double(), bias.double(), dilation=d)[0].t()


def run_conv(x, w, bias, d, slope, split, **kw):
    wp, pl = K.vocoder_pack_weight(w, 0, planes=split)
    return K.vocoder_conv(x, wp, pl, w.shape[1], w.shape[0], w.shape[2], d, slope=slope, bias=bias, bf16_split=split, **kw)


def int_operands(g, B, T, cin, cout, k):
    x = torch.randint(-3, 4, (B, T, cin), generator=g).float().to(DEV)
    w = torch.randint(-2, 3, (cout, cin, k), generator=g).float().to(DEV)
    bias = torch.randint(-4, 5, (cout,), generator=g).float().to(DEV)
    return x, w, bias


# ---- reflect conv ---------------------------------------------------------------------------------------------------------------
K3 = [(d, C) for d in (1, 3, 9) for C in (32, 64, 256)]


def conv_lengths(pad):
    return [pad + 1, 127, 128, 129, 257]


@pytest.mark.parametrize("d,C", K3)
def test_reflect_conv_integer_operands_bit_exact(d, C):
    g = torch.Generator(device="cpu").manual_seed(K3.index((d, C)))
    for T in conv_lengths(d):
        x, w, bias = int_operands(g, 1, T, C, C, 3)
        ref = reflect_conv_ref64(x[0], w, bias, d, 0.5)
        for split in (1, 0):
            out = run_conv(x, w, bias, d, 0.5, split, pad_mode="reflect")
            assert torch.equal(out[0].double(), ref), (split, T, (out[0].double() - ref).abs().max().item())


def test_reflect_conv_pre_on_the_strided_mel_view_bit_exact():
    g = torch.Generator(device="cpu").manual_seed(40)
    for T in conv_lengths(3):
        mel = torch.randint(-3, 4, (1, 80, T), generator=g).float().to(DEV)        # contiguous [B, 80, T]: the [B, T, 80] view has sxc = T
        w = torch.randint(-2, 3, (512, 80, 7), generator=g).float().to(DEV)
        bias = torch.randint(-4, 5, (512,), generator=g).float().to(DEV)
        view = mel.transpose(1, 2)
        assert not view.is_contiguous()
        ref = reflect_conv_ref64(view[0], w, bias, 1, None)
        for split in (1, 0):
            out = run_conv(view, w, bias, 1, None, split, pad_mode="reflect")
            assert torch.equal(out[0].double(), ref), (split, T)
            assert torch.equal(out, run_conv(view.contiguous(), w, bias, 1, None, split, pad_mode="reflect"))


@pytest.mark.parametrize("k,d,cin,cout", [(3, 1, 32, 32), (3, 3, 64, 64), (3, 9, 256, 256), (7, 1, 80, 512)])
def test_reflect_conv_ragged_ends_and_nan_padding(k, d, cin, cout):
    """B = 3 with ends at pad + 1, 128 and 129 rows (129: one valid row in the second tile, whose halo reflects back into the first),
    NaN in every padded row: each utterance equals float64 of itself alone and its own B = 1 call, bit for bit"""
    pad = d * (k - 1) // 2
    ends = [pad + 1, 128, 129]
    g = torch.Generator(device="cpu").manual_seed(50 + d + k)
    x, w, bias = int_operands(g, 3, 131, cin, cout, k)
    if k == 7:                                               # the first conv reads the mel's [B, T, 80] view of a [B, 80, T] tensor
        x = x.transpose(1, 2).contiguous().transpose(1, 2)
    for b, n in enumerate(ends):
        x[b, n:] = NAN
    lens = torch.tensor(ends, dtype=torch.int32, device=DEV)
    for split in (1, 0):
        out = run_conv(x, w, bias, d, 0.5, split, pad_mode="reflect", lens=lens, len_mul=1,
                       out=torch.full((3, 131, cout), 7.0, device=DEV))
        for b, n in enumerate(ends):
            assert torch.equal(out[b, :n].double(), reflect_conv_ref64(x[b, :n], w, bias, d, 0.5)), (split, b)
            assert torch.equal(out[b, :n], run_conv(x[b:b + 1, :n].contiguous(), w, bias, d, 0.5, split, pad_mode="reflect")[0])
            assert out[b, n:].eq(7.0).all()                                         # rows beyond the end are not written


@pytest.mark.parametrize("d,C", K3)
def test_reflect_conv_random_vs_fp64(d, C):
    g = torch.Generator(device="cpu").manual_seed(100 + K3.index((d, C)))
    for T in (d + 1, 129, 257):
        x = torch.randn(1, T, C, generator=g).to(DEV)
        w = (torch.randn(C, C, 3, generator=g) / (C * 3) ** 0.5).to(DEV)
        bias = torch.randn(C, generator=g).to(DEV)
        ref = reflect_conv_ref64(x[0], w, bias, d, 0.2)
        e = {split: (run_conv(x, w, bias, d, 0.2, split, pad_mode="reflect")[0].double() - ref).abs().max().item() for split in (1, 0)}
        floor = ULP * ref.abs().max().item()
        assert e[0] <= 16 * floor * max(1.0, (C * 3) ** 0.5), e
        assert e[1] <= 1.25 * e[0] + floor, e


def test_reflect_rejections():
    x = torch.zeros(1, 9, 32, device=DEV)
    w = torch.zeros(32, 32, 3, device=DEV)
    wp, _ = K.vocoder_pack_weight(w, 0, planes=False)
    lib = _lib.load()
    d = _lib.VconvMelganDesc()                                # the C entry point's own checks (the wrapper has the same ones in front)
    K._vocoder_conv_desc("t", d.conv, torch.float32, ("w", "R", "out"), x, wp, 32, 32, 3, 9, 0, None, None, None, None, 1.0, 0.0, None, 1)
    d.pad_mode = 1
    assert lib.ctts_vocoder_conv_melgan(ctypes.byref(d), None) != 0 and b"reflection needs T" in lib.ctts_last_error()
    d.pad_mode = 2
    assert lib.ctts_vocoder_conv_melgan(ctypes.byref(d), None) != 0 and b"pad_mode" in lib.ctts_last_error()
    wt, _ = K.vocoder_pack_weight(torch.zeros(32, 32, 4, device=DEV), 2, planes=False)
    d = _lib.VconvMelganDesc()
    K._vocoder_conv_desc("t", d.conv, torch.float32, ("w", "R", "out"), x, wt, 32, 32, 4, 1, 2, None, None, None, None, 1.0, 0.0, None, 1)
    d.pad_mode = 1
    assert lib.ctts_vocoder_conv_melgan(ctypes.byref(d), None) != 0 and b"Conv1d only" in lib.ctts_last_error()
    with pytest.raises(_lib.CttsError, match="reflection needs T"):
        K.vocoder_post(torch.zeros(1, 3, 32, device=DEV), torch.zeros(7, 32, device=DEV), torch.zeros(1, device=DEV), 0.2, pad_mode="reflect")


# ---- two-operand 1x1 tail -------------------------------------------------------------------------------------------------------
def tail_ref64(t, x2, w1, w2, bias, slope):
    return lrelu64(t, slope) @ w1[:, :, 0].double().t() + x2.double() @ w2[:, :, 0].double().t() + bias.double()


def run_tail(t, x2, w1, w2, bias, slope, split, **kw):
    wp, pl = K.vocoder_pack_weight(w1, planes=split, weight2=w2)
    return K.vocoder_conv(t, wp, pl, w1.shape[1], w1.shape[0], 1, slope=slope, bias=bias, bf16_split=split, x2=x2, **kw)


@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_two_operand_tail(C):
    g = torch.Generator(device="cpu").manual_seed(200 + C)
    for T in (1, 129):
        t = torch.randint(-3, 4, (2, T, C), generator=g).float().to(DEV)
        x2 = torch.randint(-3, 4, (2, T, C), generator=g).float().to(DEV)
        w1 = torch.randint(-2, 3, (C, C, 1), generator=g).float().to(DEV)
        w2 = torch.randint(-2, 3, (C, C, 1), generator=g).float().to(DEV)
        bias = torch.randint(-4, 5, (C,), generator=g).float().to(DEV)
        ref = tail_ref64(t, x2, w1, w2, bias, 0.5)
        for split in (1, 0):
            out = run_tail(t, x2, w1, w2, bias, 0.5, split)
            assert torch.equal(out.double(), ref), (split, T)                       # x2 is NOT activated: negative x2 entries would differ
        t, x2 = torch.randn(2, T, C, generator=g).to(DEV), torch.randn(2, T, C, generator=g).to(DEV)
        w1, w2 = ((torch.randn(C, C, 1, generator=g) / (2 * C) ** 0.5).to(DEV) for _ in range(2))
        bias = torch.randn(C, generator=g).to(DEV)
        ref = tail_ref64(t, x2, w1, w2, bias, 0.2)
        e = {split: (run_tail(t, x2, w1, w2, bias, 0.2, split).double() - ref).abs().max().item() for split in (1, 0)}
        floor = ULP * ref.abs().max().item()
        assert e[0] <= 16 * floor * max(1.0, (2 * C) ** 0.5), e                     # K = the sum of both inputs
        assert e[1] <= 1.25 * e[0] + floor, e


def test_two_operand_tail_unequal_odd_channels_strided_x2_and_ragged():
    """Cin = 40 and Cin2 = 70 (neither a multiple of 32, the scalar staging path), x2 a column slice of a wider tensor, lens with NaN
    beyond each end, and the three-launch form (shortcut, then R=) as a second reference"""
    g = torch.Generator(device="cpu").manual_seed(9)
    B, T, c1, c2, cout = 3, 131, 40, 70, 48
    t = torch.randint(-3, 4, (B, T, c1), generator=g).float().to(DEV)
    wide = torch.randint(-3, 4, (B, T, c2 + 5), generator=g).float().to(DEV)
    x2 = wide[:, :, 3:3 + c2]
    w1 = torch.randint(-2, 3, (cout, c1, 1), generator=g).float().to(DEV)
    w2 = torch.randint(-2, 3, (cout, c2, 1), generator=g).float().to(DEV)
    bias = torch.randint(-4, 5, (cout,), generator=g).float().to(DEV)
    ends = [1, 128, 129]
    lens = torch.tensor(ends, dtype=torch.int32, device=DEV)
    ref = tail_ref64(t, x2, w1, w2, bias, 0.5)
    for b, n in enumerate(ends):
        t[b, n:] = NAN
        wide[b, n:] = NAN
    for split in (1, 0):
        out = run_tail(t, x2, w1, w2, bias, 0.5, split, lens=lens, len_mul=1, out=torch.full((B, T, cout), 7.0, device=DEV))
        sc = run_conv(x2, w2, torch.zeros_like(bias), 1, None, split, lens=lens, len_mul=1, out=torch.zeros(B, T, cout, device=DEV))
        three = run_conv(t, w1, bias, 1, 0.5, split, R=sc, lens=lens, len_mul=1, out=torch.full((B, T, cout), 7.0, device=DEV))
        for b, n in enumerate(ends):
            assert torch.equal(out[b, :n].double(), ref[b, :n]) and out[b, n:].eq(7.0).all(), (split, b)
        assert torch.equal(out, three)
    with pytest.raises(_lib.CttsError, match="does not match the layer"):
        wp, pl = K.vocoder_pack_weight(w1, planes=False)
        K.vocoder_conv(t, wp, pl, c1, cout, 1, bf16_split=0, x2=x2)                  # a one-operand pack is too narrow for K = Cin + Cin2


# ---- reflect post ---------------------------------------------------------------------------------------------------------------
def post_ref64(x, w, bias, slope):
    """x [T, C] of one utterance, w [k, C] -> (float64 result [T], error bar): a chain of n = k C fp32 fmas errs by at most n / 2 ULP
    of its largest partial sum, which sum |x| |w| + |bias| bounds; tanh has slope <= 1 and tanhf is given 4 ULP of its result <= 1"""
    k, C = w.shape
    xp = F.pad(lrelu64(x, slope).t()[None], ((k - 1) // 2, (k - 1) // 2), mode="reflect")
    mag = F.conv1d(xp.abs(), w.double().abs().t()[None], bias.double().abs()).max().item()
    return torch.tanh(F.conv1d(xp, w.double().t()[None], bias.double()))[0, 0], (k * C / 2 * max(1.0, mag) + 4) * ULP


def test_reflect_post_dense_and_ragged():
    g = torch.Generator(device="cpu").manual_seed(300)
    C, k, Ts = 32, 7, [4, 255, 256, 257]
    w = (torch.randn(k, C, generator=g) / (C * k) ** 0.5).to(DEV)
    bias = torch.randn(1, generator=g).to(DEV)
    for T in Ts:
        x = torch.randn(2, T, C, generator=g).to(DEV)
        out = K.vocoder_post(x, w, bias, 0.2, pad_mode="reflect")
        assert out.shape == (2, 1, T)
        for b in range(2):
            ref, bar = post_ref64(x[b], w, bias, 0.2)
            assert (out[b, 0].double() - ref).abs().max().item() <= bar
    x = torch.randn(len(Ts) + 1, 300, C, generator=g).to(DEV)
    ends = Ts + [0]
    for b, n in enumerate(ends):
        x[b, n:] = NAN
    lens = torch.tensor(ends, dtype=torch.int32, device=DEV)
    out = K.vocoder_post(x, w, bias, 0.2, lens=lens, len_mul=1, pad_mode="reflect", out=torch.full((len(ends), 1, 300), 7.0, device=DEV))
    for b, n in enumerate(ends):
        if n:
            assert torch.equal(out[b, 0, :n], K.vocoder_post(x[b:b + 1, :n].contiguous(), w, bias, 0.2, pad_mode="reflect")[0, 0])
            ref, bar = post_ref64(x[b, :n], w, bias, 0.2)
            assert (out[b, 0, :n].double() - ref).abs().max().item() <= bar
        assert out[b, 0, n:].eq(0.0).all()                                           # exact zeros from Tb on
    x = torch.randn(1, 64, C, generator=g).to(DEV)                                   # len_mul: 5 frames of 8 rows
    out = K.vocoder_post(x, w, bias, 0.2, lens=torch.tensor([5], dtype=torch.int32, device=DEV), len_mul=8, pad_mode="reflect")
    assert torch.equal(out[0, 0, :40], K.vocoder_post(x[:, :40].contiguous(), w, bias, 0.2, pad_mode="reflect")[0, 0])
    assert out[0, 0, 40:].eq(0.0).all()


# ---- generator ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recipe():
    """the recipe weights, once: (state dict, float64 folded weights on the device)"""
    sd = MR.recipe_state_dict()
    return sd, MR.fold_state_dict(sd, dtype=torch.float64, device=DEV)


def _generator(sd):
    g = melgan.Generator()
    g.load_state_dict(sd)
    return g.eval().to(DEV)


def test_generator_vs_fp64_restatement(arith, recipe):
    """e = the native forward's largest error against float64, e32 = that of the stock-torch fp32 CPU forward on the same input;
    the bar is e <= 4 e32 (a wrong reflection or a missed activation is off by >= 1e-2)"""
    sd, W64 = recipe
    mel = torch.randn(3, 80, 9, generator=torch.Generator().manual_seed(2))
    ref = MR.generator_forward(W64, mel.double().to(DEV)).cpu()
    with torch.no_grad():
        e32 = (MR.generator_forward(MR.fold_state_dict(sd, dtype=torch.float32), mel).double() - ref).abs().max().item()
    out = _generator(sd)(mel.to(DEV)).cpu()
    assert out.shape == (3, 1, 256 * 9) and not out.requires_grad
    e = (out.double() - ref).abs().max().item()
    print(f"MelGAN B=3 T=9 ({'split' if arith else 'fp32 MFMA'}): native err e = {e:.3e}, CPU fp32 err e32 = {e32:.3e}, bar 4 e32 = "
          f"{4 * e32:.3e}, wav std {ref.std().item():.3f}, peak {ref.abs().max().item():.3f}")
    assert e <= 4 * e32, (e, e32)


def test_ragged_generator_rows_equal_their_own_calls(arith, recipe):
    sd, W64 = recipe
    g = _generator(sd)
    mel = torch.randn(3, 80, 12, generator=torch.Generator().manual_seed(5)).to(DEV)
    ends = [12, 4, 7]
    for b, n in enumerate(ends):
        mel[b, :, n:] = NAN
    wav = g(mel, lens=torch.tensor(ends, device=DEV))                               # int64, as the acoustic model's mel_lens
    assert wav.shape == (3, 1, 256 * 12)
    for b, n in enumerate(ends):
        assert torch.equal(wav[b, 0, :256 * n], g(mel[b:b + 1, :, :n])[0, 0]), b
        assert wav[b, 0, 256 * n:].eq(0.0).all(), b
    ref = MR.generator_forward(W64, mel[2:3, :, :7].double())
    assert (wav[2:3, :, :256 * 7].double() - ref).abs().max().item() <= 2e-5
    short = g(mel[:2, :, :6], lens=[3, 0])                                           # too short to reflect: all-zero rows
    assert short.shape == (2, 1, 256 * 6) and short.eq(0.0).all()
    assert g(mel[:2, :, :3], lens=[3, 2]).eq(0.0).all()
    with pytest.raises(_lib.CttsError, match="at least 4 frames"):
        g(mel[:1, :, :3])


def test_weight_forms_cache_and_vocoder_object(arith, recipe):
    sd, _ = recipe
    g = _generator(sd)
    mel = torch.randn(2, 80, 6, generator=torch.Generator().manual_seed(6)).to(DEV)
    a = g(mel)
    assert torch.equal(a, g(mel))                                                    # no atomics: bit-reproducible
    assert torch.equal(a, g(mel.transpose(1, 2).contiguous().transpose(1, 2)))       # the channel-last layout, read through strides
    three = g._forward(mel, fused_tail=False)        # the three-launch tail, another summation order: each form is within the generator
    assert (a - three).abs().max().item() <= 1.2e-5  # test's bar of float64 (4 e32, e32 <= 1.5e-6), so the two within twice that
    with torch.no_grad():
        g.model[24].bias.add_(0.25)                                                  # an in-place edit: the cache is rebuilt
    assert not torch.equal(g(mel), a)
    g.load_state_dict(sd)
    assert torch.equal(g(mel), a)                                                    # load_state_dict rebuilds it again
    g.remove_weight_norm()
    b = g(mel)
    assert (a - b).abs().max().item() <= 2e-6                                        # folded form
    v = melgan.MelVocoder(g)
    assert torch.equal(v.inverse(mel), b.squeeze(1)) and v.mel2wav is g
    v2 = melgan.load_melgan({k: t.cpu() for k, t in g.state_dict().items()}, DEV)
    assert torch.equal(v2.inverse(mel), b.squeeze(1))
    nat = mel * math.log(10)                                                         # the acoustic model's natural-log scale
    assert torch.equal(v.inverse(nat / np.log(10)), g(nat / math.log(10)).squeeze(1))
    lens = [6, 4]
    wavs = melgan.infer_wavs(v, nat, torch.tensor(lens, device=DEV))
    full = g(nat / math.log(10), lens=lens).squeeze(1).cpu().numpy()
    assert [w.dtype for w in wavs] == [np.int16] * 2 and [len(w) for w in wavs] == [256 * 6, 256 * 4]
    for b_, n in enumerate(lens):
        assert np.array_equal(wavs[b_], (full[b_, :256 * n] * 32768.0).astype("int16"))
    assert [len(w) for w in melgan.infer_wavs(v, nat, [9, 0])] == [256 * 6, 0]       # min(len, T)
