"""GPU: the vocoder's fp16 mode (csrc/vocoder_h.hip, include/ctts.h "fp16 mode") - the conv kernel bit-exactly on integer operands and
within its derived rounding bound on random ones, saturation, subnormals, and a Generator called as g(mel, lens, precision="fp16") against
the float64 restatement with bars computed here from the CPU emulation of the contract (tests/hifigan_half_emulation.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import kernels as K  # noqa: E402
from ctts_amd.vocoder import AttrDict, Generator  # noqa: E402
import hifigan_restate as R  # noqa: E402
import hifigan_half_emulation as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(ROOT, "tests", "golden")
V1 = dict(upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], resblock="1")
TS = [1, 5, 77, 1000, 8195]
CASES = [(k, d, c) for k in (3, 7, 11) for d in (1, 3, 5) for c in (32, 64, 128, 256)]
UPS = [(512, 256, 16, 8), (256, 128, 16, 8), (128, 64, 4, 2), (64, 32, 4, 2)]
SUB = 2.0 ** -24                     # the fp16 subnormal step


def operand64(x, slope):
    """float64 of the MFMA operand fp16(leaky_relu(float32(x), slope)) of an fp16 (or fp32: the mel) tensor x"""
    x32 = x.float()
    if slope is not None:
        x32 = torch.where(x32 > 0, x32, x32 * slope)
    return x32.clamp(-65504.0, 65504.0).half().double()


def conv_ref64(a, w, bias, d, R_=None, old=None, alpha=1.0, beta=0.0, u=0):
    """float64 on the device.  a: operand [B, T, Cin] float64, w float64 Conv1d [Cout, Cin, k] or (u > 0) ConvTranspose1d [Cin, Cout, k]
    -> (beta * old + alpha * (conv + bias + R), sum |a||w| + |bias| + |R|), both [B, T_out, Cout]"""
    def conv(a_, w_):
        if u:
            return F.conv_transpose1d(a_.transpose(1, 2), w_, None, u, (w_.shape[2] - u) // 2).transpose(1, 2)
        return F.conv1d(a_.transpose(1, 2), w_, None, 1, d * (w_.shape[2] - 1) // 2, d).transpose(1, 2)
    acc, mag = conv(a, w), conv(a.abs(), w.abs())
    if bias is not None:
        acc, mag = acc + bias.double(), mag + bias.double().abs()
    if R_ is not None:
        acc, mag = acc + R_.double(), mag + R_.double().abs()
    acc = alpha * acc
    if beta != 0.0:
        acc = beta * old.double() + acc
    return acc, mag


def run_conv(x, w, bias, d, slope, u=0, **kw):
    """x fp16 / fp32 [B, T, Cin] on the device, w fp32 master weight (rounded to fp16 by the packer)"""
    wp = K.vocoder_pack_weight_h(w, u)
    cin, cout = (w.shape[0], w.shape[1]) if u else (w.shape[1], w.shape[0])
    return K.vocoder_conv_h(x, wp, cin, cout, w.shape[2], d, transposed_u=u, slope=slope, bias=bias, **kw)


def sparse_even_weight(shape, kdim_elems, g, nnz=300):
    """weights in {-2, 0, 2}, about nnz / 2 non-zeros among the K = taps x Cin products of an output column, so that with operands of
    magnitude <= 3 the sum of magnitudes stays far below 2048 (integer_case asserts it): every partial sum is an exact even integer"""
    keep = min(1.0, nnz / (2.0 * kdim_elems))
    w = (torch.randint(0, 2, shape, generator=g) * 4 - 2).float() * (torch.rand(shape, generator=g) < keep)
    return w


def integer_case(B, T, cin, cout, k, d, u, g):
    x = torch.tensor([-4.0, -2.0, 0.0, 1.0, 2.0, 3.0])[torch.randint(0, 6, (B, T, cin), generator=g)]    # slope 0.5 -> integers, |a| <= 3
    wshape = (cin, cout, k) if u else (cout, cin, k)
    w = sparse_even_weight(wshape, cin * (k // u if u else k), g)
    Tout = T * u if u else T
    bias = (torch.randint(-2, 3, (cout,), generator=g) * 2).float()
    Rr = (torch.randint(-2, 3, (B, Tout, cout), generator=g) * 2).float()
    old = torch.randint(-4, 5, (B, Tout, cout), generator=g).float()
    x, w, bias, Rr, old = (t.to(DEV) for t in (x, w, bias, Rr, old))
    ref, mag = conv_ref64(operand64(x.half(), 0.5), w.double(), bias, d, Rr, old, 0.5, 2.0, u)
    # the premise of the exactness claim, checked: every partial sum (bounded by the sum of magnitudes) and every output is an integer
    # of magnitude <= 2048 - exact in fp16 and in fp32, in any order
    assert mag.max().item() <= 2048 and ref.abs().max().item() <= 2048 and torch.equal(ref, ref.round())
    out = run_conv(x.half(), w, bias, d, 0.5, u, R=Rr.half(), out=old.half(), alpha=0.5, beta=2.0)
    assert out.dtype == torch.float16
    return out, ref


@pytest.mark.parametrize("k,d,C", CASES)
def test_conv_integer_operands_bit_exact(k, d, C):
    i = CASES.index((k, d, C))
    g = torch.Generator(device="cpu").manual_seed(i)
    for B, T in ((1, TS[i % 5]), (3, TS[(i + 2) % 5])):
        out, ref = integer_case(B, T, C, C, k, d, 0, g)
        assert torch.equal(out.double(), ref), (B, T, (out.double() - ref).abs().max().item())


@pytest.mark.parametrize("cin,cout,k,u", UPS)
def test_transposed_conv_integer_operands_bit_exact(cin, cout, k, u):
    g = torch.Generator(device="cpu").manual_seed(cin + k)
    for B, T in ((1, 1), (2, 5), (3, 77), (1, 1000), (2, 8195)):
        out, ref = integer_case(B, T, cin, cout, k, 1, u, g)
        assert out.shape == (B, T * u, cout)
        assert torch.equal(out.double(), ref), (B, T, (out.double() - ref).abs().max().item())


@pytest.mark.parametrize("C,k,d", [(32, 11, 5), (64, 7, 3), (128, 3, 1)])
def test_large_batch_keeps_the_bits(C, k, d):
    """a large batch (>= 1024 tiles of 128 rows per launch): exact on integers, and every utterance bit-equal to its own B = 1 call
    whatever tile height the library runs (CTTS_VOCODER_H_BM=256 selects the 256-row tiles)"""
    g = torch.Generator(device="cpu").manual_seed(C)
    B, T = 16 if C < 128 else 32, 8195
    out, ref = integer_case(B, T, C, C, k, d, 0, g)
    assert torch.equal(out.double(), ref)
    x = torch.randn(B, T, C, generator=g).half().to(DEV)
    w = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    bias = torch.randn(C, generator=g).to(DEV)
    full = run_conv(x, w, bias, d, 0.1)
    for b in (0, B - 1):
        assert torch.equal(full[b:b + 1], run_conv(x[b:b + 1], w, bias, d, 0.1))


def bound(ref, mag, Kdim):
    """|err| <= 2^-11 |ref| (the one rounding of the stored output) + K 2^-24 sum|a||b| (fp32 accumulation in any order; the sum takes
    |bias| and |R| in for the epilogue's fp32 additions) + one fp16 subnormal step"""
    return 2.0 ** -11 * ref.abs() + Kdim * 2.0 ** -24 * mag + SUB


@pytest.mark.parametrize("k,d,C", CASES)
def test_conv_random_vs_fp64_on_rounded_operands(k, d, C):
    i = CASES.index((k, d, C))
    g = torch.Generator(device="cpu").manual_seed(100 + i)
    for B, T in ((3, TS[(i + 1) % 5]), (1, TS[(i + 3) % 5])):
        x = torch.randn(B, T, C, generator=g).half().to(DEV)
        w = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
        bias = torch.randn(C, generator=g).to(DEV)
        Rr = torch.randn(B, T, C, generator=g).half().to(DEV)
        ref, mag = conv_ref64(operand64(x, 0.1), w.half().double(), bias, d, Rr)
        out = run_conv(x, w, bias, d, 0.1, R=Rr)
        err = (out.double() - ref).abs()
        lim = bound(ref, mag, C * k)
        print(f"k={k} d={d} C={C} B={B} T={T}: max err {err.max().item():.3e}, largest err / bound {(err / lim).max().item():.3f}")
        assert (err <= lim).all(), (B, T, (err / lim).max().item())


@pytest.mark.parametrize("cin,cout,k,u", UPS)
def test_transposed_conv_random_vs_fp64_on_rounded_operands(cin, cout, k, u):
    g = torch.Generator(device="cpu").manual_seed(cin + k)
    w = (torch.randn(cin, cout, k, generator=g) / (cin * k / u) ** 0.5).to(DEV)
    bias = torch.randn(cout, generator=g).to(DEV)
    for B, T in ((2, 1), (3, 5), (2, 37), (2, 77), (1, 1000), (2, 8195)):
        x = torch.randn(B, T, cin, generator=g).half().to(DEV)
        ref, mag = conv_ref64(operand64(x, 0.1), w.half().double(), bias, 1, u=u)
        out = run_conv(x, w, bias, 1, 0.1, u)
        err, lim = (out.double() - ref).abs(), bound(ref, mag, cin * k // u)
        print(f"up {cin}->{cout} k={k} u={u} B={B} T={T}: max err {err.max().item():.3e}, largest err / bound {(err / lim).max().item():.3f}")
        assert (err <= lim).all(), (B, T)


@pytest.mark.parametrize("cin,cout,k,u", UPS)
def test_transposed_conv_ragged_rows_equal_their_own_call(cin, cout, k, u):
    """the polyphase scatter with lens at a long T: utterance b's rows are bit-equal to a B = 1 call on x[b, :Tb] (tiles anchored at
    row 0, ends inside a tile, on a tile boundary and beyond T), NaN beyond the end is never read"""
    g = torch.Generator(device="cpu").manual_seed(cin + u)
    T, len_mul = 2100, 4
    lens = [525, 256, 130, 1, 0, 9999]                        # x len_mul: 2100 (= T), 1024 (a tile boundary), 520, 4, 0, clamped to T
    B = len(lens)
    x = torch.randn(B, T, cin, generator=g).half().to(DEV)
    w = (torch.randn(cin, cout, k, generator=g) / (cin * k / u) ** 0.5).to(DEV)
    bias = torch.randn(cout, generator=g).to(DEV)
    rows = [min(max(n, 0) * len_mul, T) for n in lens]
    for b, n in enumerate(rows):
        x[b, n:] = float("nan")
    out = torch.full((B, T * u, cout), 7.0, dtype=torch.float16, device=DEV)
    wp = K.vocoder_pack_weight_h(w, u)
    K.vocoder_conv_h(x, wp, cin, cout, k, 1, transposed_u=u, slope=0.1, bias=bias, out=out,
                     lens=torch.tensor(lens, dtype=torch.int32, device=DEV), len_mul=len_mul)
    for b, n in enumerate(rows):
        if n:
            alone = K.vocoder_conv_h(x[b:b + 1, :n], wp, cin, cout, k, 1, transposed_u=u, slope=0.1, bias=bias)
            assert torch.equal(out[b, :n * u], alone[0]), b
        assert torch.equal(out[b, n * u:], torch.full_like(out[b, n * u:], 7.0)), b      # rows beyond the end are not written


def test_conv_pre_reads_the_fp32_mel_through_its_strides():
    g = torch.Generator(device="cpu").manual_seed(7)
    mel = torch.randn(3, 80, 77, generator=g).to(DEV)             # contiguous [B, 80, T]: its [B, T, 80] view has sxc = T
    w = (torch.randn(512, 80, 7, generator=g) / 24).to(DEV)
    bias = torch.randn(512, generator=g).to(DEV)
    a = run_conv(mel.transpose(1, 2), w, bias, 1, None)
    b = run_conv(mel.transpose(1, 2).contiguous(), w, bias, 1, None)
    c = run_conv(mel.transpose(1, 2).contiguous().half(), w, bias, 1, None)     # the staging's rounding, done by the caller
    assert torch.equal(a, b) and torch.equal(a, c)
    ref, mag = conv_ref64(operand64(mel.transpose(1, 2), None), w.half().double(), bias, 1)
    assert ((a.double() - ref).abs() <= bound(ref, mag, 80 * 7)).all()


def test_saturation_stores_the_largest_finite_value():
    C, T = 64, 300
    x = torch.full((2, T, C), 100.0, dtype=torch.float16, device=DEV)
    x[1] = -100.0
    w = torch.full((C, C, 3), 8.0, device=DEV)
    w[C // 2:] = -8.0
    out = run_conv(x, w, None, 1, None)                           # |sum| = 100 x 8 x 192 = 153600 > 65504
    assert torch.isfinite(out).all()
    assert torch.equal(out[0, 5, :C // 2], torch.full((C // 2,), 65504.0, dtype=torch.float16, device=DEV))
    assert torch.equal(out[0, 5, C // 2:], torch.full((C // 2,), -65504.0, dtype=torch.float16, device=DEV))
    assert torch.equal(out[1], -out[0])
    big = torch.full((2, T, C), 60000.0, dtype=torch.float16, device=DEV)
    z = torch.zeros(C, C, 3, device=DEV)
    out = run_conv(x, z, None, 1, None, R=big, out=big.clone(), alpha=1.0, beta=1.0)     # the epilogue alone: 60000 + 60000
    assert torch.equal(out, torch.full_like(out, 65504.0))
    out = run_conv(torch.full((1, 4, 80), 1e30, device=DEV), torch.ones(32, 80, 7, device=DEV), None, 1, None)   # an fp32 input beyond fp16
    assert torch.isfinite(out).all() and out.max().item() == 65504.0


def test_conv_subnormal_operands():
    """Records what v_mfma_f32_32x32x16_f16 does with fp16 subnormal operands and asserts what include/ctts.h states: they are NOT
    flushed - subnormal weights, subnormal inputs (before and after the on-load leaky_relu) and a subnormal stored result are exact."""
    C, T = 32, 40
    sub_w = torch.zeros(C, C, 3, device=DEV)
    sub_w[:, :, 1] = torch.eye(C, device=DEV) * (5 * SUB)         # a subnormal weight: out[t, c] = 5 x 2^-24 x[t, c]
    x = torch.full((1, T, C), 1024.0, dtype=torch.float16, device=DEV)
    a = run_conv(x, sub_w, None, 1, None)                         # normal x subnormal -> 5 x 2^-14
    nw = torch.zeros(C, C, 3, device=DEV)
    nw[:, :, 1] = torch.eye(C, device=DEV) * 1024.0
    xs = torch.full((1, T, C), 3 * SUB, dtype=torch.float16, device=DEV)
    b = run_conv(xs, nw, None, 1, None)                           # subnormal x normal -> 3 x 2^-14
    xn = torch.full((1, T, C), -6 * SUB, dtype=torch.float16, device=DEV)
    c = run_conv(xn, nw, None, 1, 0.5)                            # leaky_relu of a subnormal: -3 x 2^-24, x 1024
    one = torch.zeros(C, C, 3, device=DEV)
    one[:, :, 1] = torch.eye(C, device=DEV)
    d = run_conv(xs, one, None, 1, None)                          # a subnormal result, stored as such
    got = [t.double().unique().tolist() for t in (a, b, c, d)]
    print("subnormal operands: weight", got[0], "input", got[1], "activated input", got[2], "stored", got[3],
          "(flushed operands would give 0.0)")
    assert got == [[5 * 2.0 ** -14], [3 * 2.0 ** -14], [-3 * 2.0 ** -14], [3 * SUB]]


# ---- network level -----------------------------------------------------------------------------------------------------------------
def _g17():
    return R.load_g17(os.path.join(GOLD, "g17_hifigan_small.npz"))


def _g17_generator():
    z, h, sd = _g17()
    g = Generator(AttrDict(h))
    g.load_state_dict(sd)
    return g.eval().to(DEV), z, h, sd


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


def _against_fp64(name, g, h, sd, mel):
    """the native fp16 wav against the float64 restatement; the bars are the errors of the contract's CPU emulation with float32
    accumulation in two summation orders: rms <= 1.25 x the larger emulated rms, max <= 2 x the larger emulated max"""
    ref = R.generator_forward(R.fold_state_dict(sd, dtype=torch.float64, device=DEV), h, mel.double().to(DEV)).cpu()
    W32 = R.fold_state_dict(sd, dtype=torch.float32)
    emu = {}
    with torch.no_grad():
        for rev in (False, True):
            e = E.generator_forward_half(W32, h, mel, acc_dtype=torch.float32, reverse_channels=rev).double() - ref
            emu[rev] = (e.pow(2).mean().sqrt().item(), e.abs().max().item())
    out = g(mel.to(DEV), precision="fp16")
    assert out.dtype == torch.float32 and out.shape == ref.shape and torch.isfinite(out).all()
    e = out.cpu().double() - ref
    rms, mx = e.pow(2).mean().sqrt().item(), e.abs().max().item()
    snr = 20 * np.log10(ref.std().item() / rms)
    print(f"{name}: native fp16 vs float64 rms {rms:.3e} max {mx:.3e} ({snr:.1f} dB, wav std {ref.std().item():.3f}); emulation "
          f"natural order rms {emu[False][0]:.3e} max {emu[False][1]:.3e}, reversed rms {emu[True][0]:.3e} max {emu[True][1]:.3e}")
    assert rms <= 1.25 * max(emu[False][0], emu[True][0]), (rms, emu)
    assert mx <= 2.0 * max(emu[False][1], emu[True][1]), (mx, emu)


def test_g17_fp16_vs_fp64_restatement():
    g, z, h, sd = _g17_generator()
    _against_fp64("g17", g, h, sd, torch.from_numpy(z["mel"]))


def test_v1_size_fp16_vs_fp64_restatement():
    g = _v1_generator()
    sd = {k: v.detach().clone() for k, v in g.state_dict().items()}
    mel = torch.randn(2, 80, 64, generator=torch.Generator().manual_seed(2))
    mel[1, :, 37:] = -4.0
    _against_fp64("V1 B=2 T=64", g.to(DEV), V1, sd, mel)


def test_ragged_fp16_is_each_utterance_alone():
    g, _, h, _ = _g17_generator()
    z = np.load(os.path.join(GOLD, "g20_hifigan_ragged.npz"))
    lens = [int(v) for v in z["mel_lens"]]
    assert lens == [32, 13, 1, 27]
    mel = torch.from_numpy(z["mel"]).to(DEV)
    B, _, T = mel.shape
    for b, n in enumerate(lens):
        mel[b, :, n:] = float("nan")                             # the padded frames are never read
    wav = g(mel, lens=lens, precision="fp16")
    assert wav.shape == (B, 1, 256 * T) and wav.dtype == torch.float32
    for b, n in enumerate(lens):
        alone = g(mel[b:b + 1, :, :n], precision="fp16")
        assert torch.equal(wav[b, 0, :256 * n], alone[0, 0]), b
        assert torch.equal(wav[b, 0, 256 * n:], torch.zeros(256 * (T - n), device=DEV)), b
    assert torch.equal(g(mel, lens=torch.tensor(lens, device=DEV), precision="fp16"), wav)      # int64 on the device
    # lens[b] = 0 gives a zero row, lens[b] > T behaves as T
    mel2 = torch.from_numpy(z["mel"]).to(DEV)
    dense = g(mel2, precision="fp16")
    wav2 = g(mel2, lens=[0, T + 9, T, 0], precision="fp16")
    assert torch.equal(wav2[0], torch.zeros_like(wav2[0])) and torch.equal(wav2[3], torch.zeros_like(wav2[3]))
    assert torch.equal(wav2[1], dense[1]) and torch.equal(wav2[2], dense[2])


def test_fp16_reproducible_strided_and_mixed_with_fp32():
    g, z, h, sd = _g17_generator()
    mel = torch.from_numpy(z["mel"]).to(DEV)
    a = g(mel, precision="fp16")
    assert torch.equal(a, g(mel, precision="fp16"))              # two calls
    cl = mel.transpose(1, 2).contiguous()                        # the model's channel-last [B, T, 80]; its transposed view is not contiguous
    view = cl.transpose(1, 2)
    assert not view.is_contiguous() and torch.equal(g(view, precision="fp16"), a)
    f = g(mel)                                                   # default: fp32
    assert torch.equal(f, g(mel, precision="fp32")) and not torch.equal(f, a)
    assert (f - a).abs().max().item() < 0.1
    assert torch.equal(g(mel, precision="fp16"), a)              # fp16, fp32, fp16: the first result again
    fresh, *_ = _g17_generator()
    assert torch.equal(fresh(mel), f)                            # the fp32 mode never saw the fp16 pack
    key32, key16 = g._packs["fp32"][0], g._packs["fp16"][0]
    g(mel, precision="fp16"), g(mel), g(mel, precision="fp16")
    assert g._packs["fp32"][0] is key32 and g._packs["fp16"][0] is key16     # neither mode rebuilt the other's (or its own) cache
    g.default_precision = "fp16"
    assert torch.equal(g(mel), a)


def test_both_precisions_launch_the_same_layer_schedule(monkeypatch):
    """every launch of g(mel) and of g(mel, precision="fp16"), dense and ragged, recorded at the kernel wrappers: the two precisions run
    the same layers with the same epilogue terms in the same order, 1 + nu + 6 nu nk + 1 of them"""
    import inspect
    g, z, h, _ = _g17_generator()
    z20 = np.load(os.path.join(GOLD, "g20_hifigan_ragged.npz"))
    lens = [int(v) for v in z20["mel_lens"]]
    assert lens == [32, 13, 1, 27]
    log = []

    def record(name):
        fn = getattr(K, name)
        sig = inspect.signature(fn)

        def wrapper(*args, **kw):
            a = sig.bind(*args, **kw)
            a.apply_defaults()
            a = a.arguments
            if "Cin" in a:
                log.append((a["Cin"], a["Cout"], a["k"], a["dil"], a["transposed_u"], a["slope"], a["R"] is not None, a["out"] is not None,
                            a["alpha"], a["beta"], a["len_mul"], a["lens"] is not None))
            else:                                                # conv_post: x [B, T, C], w [k, C]
                log.append((a["x"].shape[2], 1, a["w"].shape[0], 1, 0, a["slope"], False, a["out"] is not None, 1.0, 0.0, a["len_mul"],
                            a["lens"] is not None))
            return fn(*args, **kw)
        monkeypatch.setattr(K, name, wrapper)

    for name in ("vocoder_conv", "vocoder_post", "vocoder_conv_h", "vocoder_post_h"):
        record(name)
    nu, nk = g.num_upsamples, g.num_kernels
    for mel, ln in ((torch.from_numpy(z["mel"]).to(DEV), None), (torch.from_numpy(z20["mel"]).to(DEV), lens)):
        seqs = {}
        for precision in ("fp32", "fp16"):
            del log[:]
            g(mel, lens=ln, precision=precision)
            seqs[precision] = list(log)
        assert seqs["fp32"] == seqs["fp16"]
        assert len(seqs["fp32"]) == 1 + nu + 6 * nu * nk + 1
        assert all(e[-1] == (ln is not None) for e in seqs["fp32"])


def test_fp16_pack_follows_the_parameters():
    g, z, h, sd = _g17_generator()
    mel = torch.from_numpy(z["mel"]).to(DEV)
    a = g(mel, precision="fp16")
    f = g(mel)
    with torch.no_grad():
        g.conv_post.bias.add_(0.5)                               # an in-place edit bumps the version counter: both packs are rebuilt
    assert not torch.equal(g(mel, precision="fp16"), a) and not torch.equal(g(mel), f)
    g.load_state_dict(sd)
    assert torch.equal(g(mel, precision="fp16"), a) and torch.equal(g(mel), f)
    with torch.no_grad():
        g.ups[0].weight_g.mul_(1.5)
    b = g(mel, precision="fp16")
    assert not torch.equal(b, a)
    g.remove_weight_norm()                                       # new parameters: the pack is rebuilt from the folded weights
    c = g(mel, precision="fp16")
    twin, *_ = _g17_generator()                                  # the same edits on a generator that never packed anything before
    with torch.no_grad():
        twin.ups[0].weight_g.mul_(1.5)
    twin.remove_weight_norm()
    assert torch.equal(twin(mel, precision="fp16"), c) and not torch.equal(c, a)
