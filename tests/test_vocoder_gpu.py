"""GPU: the HiFi-GAN vocoder kernels (csrc/vocoder.hip) and the native Generator (vocoder.py) against float64 and against the fixtures
tests/golden/make_goldens_vocoder.py wrote from the live reference.  Both arithmetics: the exact three-way bf16 split (default) and
exact fp32 MFMA (CTTS_X6=0, kernels.gemm_bf16_split_enable(False))."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402
from ctts_amd import kernels as K  # noqa: E402
from ctts_amd.vocoder import AttrDict, Generator  # noqa: E402
import hifigan_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(ROOT, "tests", "golden")
V1 = dict(upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], resblock="1")
ULP = 2.0 ** -23


@pytest.fixture(params=[1, 0], ids=["split", "fp32"])
def arith(request):
    prev = K.gemm_bf16_split_enable(request.param)
    yield request.param
    K.gemm_bf16_split_enable(prev)


def conv_ref64(x, w, bias, d, slope, R_=None, old=None, alpha=1.0, beta=0.0):
    """float64 on the device, taps as shifted matmuls: x [B, T, Cin], w [Cout, Cin, k] -> [B, T, Cout]"""
    x = x.double()
    if slope is not None:
        x = torch.where(x > 0, x, x * slope)
    B, T, Cin = x.shape
    Cout, _, k = w.shape
    pad = d * (k - 1) // 2
    xp = F.pad(x, (0, 0, pad, pad))
    acc = torch.zeros(B, T, Cout, dtype=torch.float64, device=x.device)
    for tap in range(k):
        acc += xp[:, tap * d: tap * d + T, :] @ w[:, :, tap].double().t()
    if bias is not None:
        acc += bias.double()
    if R_ is not None:
        acc += R_.double()
    acc = alpha * acc
    if beta != 0.0:
        acc = beta * old.double() + acc
    return acc


def run_conv(x, w, bias, d, slope, split, **kw):
    wp, pl = K.vocoder_pack_weight(w, 0, planes=split)
    return K.vocoder_conv(x, wp, pl, w.shape[1], w.shape[0], w.shape[2], d, slope=slope, bias=bias, bf16_split=split, **kw)


TS = [1, 5, 77, 1000, 8195]
CASES = [(k, d, c) for k in (3, 7, 11) for d in (1, 3, 5) for c in (32, 64, 128, 256)]


@pytest.mark.parametrize("k,d,C", CASES)
def test_conv_integer_operands_bit_exact(k, d, C):
    i = CASES.index((k, d, C))
    g = torch.Generator(device="cpu").manual_seed(i)
    for B, T in ((1, TS[i % 5]), (3, TS[(i + 2) % 5])):
        x = torch.randint(-3, 4, (B, T, C), generator=g).float().to(DEV)
        w = torch.randint(-2, 3, (C, C, k), generator=g).float().to(DEV)
        bias = torch.randint(-4, 5, (C,), generator=g).float().to(DEV)
        Rr = torch.randint(-4, 5, (B, T, C), generator=g).float().to(DEV)
        old = torch.randint(-4, 5, (B, T, C), generator=g).float().to(DEV)
        ref = conv_ref64(x, w, bias, d, 0.5, Rr, old, 0.5, 2.0)
        for split in (1, 0):
            out = run_conv(x, w, bias, d, 0.5, split, R=Rr, out=old.clone(), alpha=0.5, beta=2.0)
            assert torch.equal(out.double(), ref), (split, B, T, (out.double() - ref).abs().max().item())


@pytest.mark.parametrize("k,d,C", CASES)
def test_conv_random_vs_fp64(k, d, C):
    i = CASES.index((k, d, C))
    g = torch.Generator(device="cpu").manual_seed(100 + i)
    for B, T in ((3, TS[(i + 1) % 5]), (1, TS[(i + 3) % 5])):
        x = torch.randn(B, T, C, generator=g).to(DEV)
        w = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
        bias = torch.randn(C, generator=g).to(DEV)
        Rr = torch.randn(B, T, C, generator=g).to(DEV)
        ref = conv_ref64(x, w, bias, d, 0.1, Rr)
        e = {}
        for split in (1, 0):
            out = run_conv(x, w, bias, d, 0.1, split, R=Rr)
            e[split] = (out.double() - ref).abs().max().item()
        floor = ULP * ref.abs().max().item()
        assert e[0] <= 16 * floor * max(1.0, (C * k) ** 0.5), e
        assert e[1] <= 1.25 * e[0] + floor, e


def test_conv_pre_shape_and_strided_input():
    g = torch.Generator(device="cpu").manual_seed(7)
    mel = torch.randn(3, 80, 77, generator=g).to(DEV)             # contiguous [B, 80, T]: its [B, T, 80] view has sxc = T
    w = (torch.randn(512, 80, 7, generator=g) / 24).to(DEV)
    bias = torch.randn(512, generator=g).to(DEV)
    ref = conv_ref64(mel.transpose(1, 2), w, bias, 1, None)
    for split in (1, 0):
        a = run_conv(mel.transpose(1, 2), w, bias, 1, None, split)
        b = run_conv(mel.transpose(1, 2).contiguous(), w, bias, 1, None, split)
        assert torch.equal(a, b)
        assert (a.double() - ref).abs().max().item() <= 1e-5


def test_conv_rejects_a_misshaped_or_misplaced_R():
    """R is read at out's offsets: one of another shape (here too short) would be read out of bounds, so it raises before any launch"""
    from ctts_amd import _lib
    g = torch.Generator(device="cpu").manual_seed(3)
    B, T, C, k = 1, 4, 32, 3
    x = torch.randn(B, T, C, generator=g).to(DEV)
    w = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    for split in (1, 0):
        for shape in ((B, T - 1, C), (B, T, C - 1), (T, C), (B, T, 2 * C)):
            with pytest.raises(_lib.CttsError, match="R has shape"):
                run_conv(x, w, None, 1, 0.1, split, R=torch.zeros(shape, device=DEV))
        with pytest.raises(_lib.CttsError, match="R is on cpu"):
            run_conv(x, w, None, 1, 0.1, split, R=torch.zeros(B, T, C))
        Rr = torch.randn(B, T, C, generator=g).to(DEV)
        assert (run_conv(x, w, None, 1, 0.1, split, R=Rr).double() - conv_ref64(x, w, None, 1, 0.1, Rr)).abs().max().item() <= 1e-5


@pytest.mark.parametrize("cin,cout,k,u", [(512, 256, 16, 8), (256, 128, 16, 8), (128, 64, 4, 2), (64, 32, 4, 2)])
def test_transposed_conv_vs_fp64(cin, cout, k, u):
    g = torch.Generator(device="cpu").manual_seed(cin + k)
    B, T = 2, 37
    x = torch.randn(B, T, cin, generator=g)
    w = torch.randn(cin, cout, k, generator=g) / (cin * k / u) ** 0.5
    bias = torch.randn(cout, generator=g)
    xl = torch.where(x > 0, x, 0.1 * x)
    ref = F.conv_transpose1d(xl.double().transpose(1, 2), w.double(), bias.double(), u, (k - u) // 2).transpose(1, 2)
    assert ref.shape == (B, T * u, cout)
    outs = {}
    for split in (1, 0):
        wp, pl = K.vocoder_pack_weight(w.to(DEV), u, planes=split)
        out = K.vocoder_conv(x.to(DEV), wp, pl, cin, cout, k, 1, transposed_u=u, slope=0.1, bias=bias.to(DEV), bf16_split=split).cpu()
        outs[split] = (out.double() - ref).abs()
        pad = (k - u) // 2
        edge = torch.cat([outs[split][:, :pad], outs[split][:, T * u - pad:]], 1)
        assert edge.max().item() <= 1e-5 and outs[split].max().item() <= 1e-5, split
    assert outs[1].max().item() <= 1.25 * outs[0].max().item() + ULP * ref.abs().max().item()


def _g17():
    return R.load_g17(os.path.join(GOLD, "g17_hifigan_small.npz"))


def test_generator_matches_g17_both_weight_forms(arith):
    z, h, sd = _g17()
    g = Generator(AttrDict(h))
    g.load_state_dict(sd)
    g.eval().to(DEV)
    mel = torch.from_numpy(z["mel"]).to(DEV)
    out = g(mel).cpu()
    assert out.shape == (2, 1, 256 * 32) and not out.requires_grad
    e_wn = (out - torch.from_numpy(z["wav_wn"])).abs().max().item()
    g.remove_weight_norm()
    out2 = g(mel).cpu()                                      # the cache is rebuilt from the folded parameters
    e_f = (out2 - torch.from_numpy(z["wav_folded"])).abs().max().item()
    assert e_wn <= 2e-5 and e_f <= 2e-5, (e_wn, e_f)
    assert (out - out2).abs().max().item() <= 2e-6


def _v1_generator(seed=11):
    torch.manual_seed(seed)
    g = Generator(AttrDict(V1))
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in g.named_modules():
            if hasattr(m, "weight_g"):
                m.weight_v.copy_(torch.randn(m.weight_v.shape, generator=gen))
                gain = (m.stride[0] * m.out_channels / m.in_channels) ** 0.5 if name.startswith("ups.") else (0.5 if name == "conv_post" else 1.0)
                m.weight_g.copy_(gain * (0.75 + 0.5 * torch.rand(m.weight_g.shape, generator=gen)))
                m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=gen))
    return g.eval()


def test_v1_size_vs_fp64_restatement(arith):
    g = _v1_generator()
    sd = {k: v.detach().clone() for k, v in g.state_dict().items()}
    mel = torch.randn(2, 80, 64, generator=torch.Generator().manual_seed(2))
    mel[1, :, 37:] = -4.0
    ref = R.generator_forward(R.fold_state_dict(sd, dtype=torch.float64, device=DEV), V1, mel.double().to(DEV)).cpu()
    with torch.no_grad():
        cpu32 = R.generator_forward(R.fold_state_dict(sd, dtype=torch.float32), V1, mel)
    e_cpu = (cpu32.double() - ref).abs().max().item()
    g.to(DEV)
    out = g(mel.to(DEV)).cpu()
    e = (out.double() - ref).abs().max().item()
    print(f"V1 B=2 T=64: native err {e:.3e}, CPU fp32 restatement err {e_cpu:.3e}, wav std {ref.std().item():.3f}")
    assert e <= 1e-4 and e <= 2 * e_cpu, (e, e_cpu)


def test_model_mel_view_feeds_vocoder(arith):
    from ctts_amd.configs import get_configs
    from ctts_amd.synthetic import make_batch, to_device, as_model_args
    pre, mc, tc = get_configs()
    torch.manual_seed(0)
    model = ctts_amd.CompTransTTS(pre, mc, tc).to(DEV).eval()
    args = as_model_args(to_device(make_batch([12, 9], 40, seed=4), DEV))
    with torch.no_grad():
        mel = model(*args[:4])[1]                            # postnet mel [B, T, 80], channel-last
    assert mel.is_contiguous() and mel.shape[2] == 80
    z, h, sd = _g17()
    g = Generator(AttrDict(h))
    g.load_state_dict(sd)
    g.to(DEV)
    view = mel.transpose(1, 2)                               # what utils/tools.py:342-350 hands vocoder_infer
    assert not view.is_contiguous()
    a = g(view)
    b = g(view.contiguous())
    assert torch.equal(a, b)
    ref = R.generator_forward(R.fold_state_dict(sd, dtype=torch.float64, device=DEV), h, view.double()).cpu()
    assert (a.cpu().double() - ref).abs().max().item() <= 2e-5


def test_reproducible_and_cache_invalidation(arith):
    z, h, sd = _g17()
    g = Generator(AttrDict(h))
    g.load_state_dict(sd)
    g.to(DEV)
    mel = torch.from_numpy(z["mel"]).to(DEV)
    a, b = g(mel), g(mel)
    assert torch.equal(a, b)
    with torch.no_grad():
        g.conv_post.bias.add_(0.5)                           # an in-place edit bumps the version counter: the cache is rebuilt
    c = g(mel)
    assert not torch.equal(a, c)
    g.load_state_dict(sd)
    assert torch.equal(g(mel), a)
