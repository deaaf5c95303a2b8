"""GPU: the length-aware HiFi-GAN forward, `Generator.forward(mel, lens)` (csrc/vocoder.hip's per-utterance bounds): against the live
reference's B = 1 outputs (tests/golden/g20_hifigan_ragged.npz) and, bit for bit, against the native generator called once per
utterance on the unpadded mel.  Both arithmetics, as tests/test_vocoder_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402
from ctts_amd import kernels as K  # noqa: E402
from ctts_amd import vocoder  # noqa: E402
from ctts_amd.vocoder import AttrDict, Generator  # noqa: E402
import hifigan_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(ROOT, "tests", "golden")
V1 = dict(upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], resblock="1")
BAR = 2e-5          # test_vocoder_gpu.py::test_generator_matches_g17_both_weight_forms holds the dense path to the same bar
HOP = 256


@pytest.fixture(params=[1, 0], ids=["split", "fp32"])
def arith(request):
    prev = K.gemm_bf16_split_enable(request.param)
    yield request.param
    K.gemm_bf16_split_enable(prev)


def _g17():
    return R.load_g17(os.path.join(GOLD, "g17_hifigan_small.npz"))


def _small_generator():
    _, h, sd = _g17()
    g = Generator(AttrDict(h))
    g.load_state_dict(sd)
    return g.eval().to(DEV), h, sd


def _g20():
    z = np.load(os.path.join(GOLD, "g20_hifigan_ragged.npz"))
    lens = [int(v) for v in z["mel_lens"]]
    offs = np.concatenate([[0], np.cumsum(lens)]) * HOP
    return torch.from_numpy(z["mel"]), lens, [torch.from_numpy(z["wavs"][offs[b]:offs[b + 1]]) for b in range(len(lens))]


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
    g.eval()
    g.remove_weight_norm()
    return g.to(DEV)


def _padded_mel(lens, T, seed):
    """[B, 80, T] on the device, valid frames N(0, 1), padded frames -4 +- 0.3 (non-zero, as a PostNet leaves them)"""
    gen = torch.Generator().manual_seed(seed)
    mel = torch.randn(len(lens), 80, T, generator=gen)
    for b, n in enumerate(lens):
        mel[b, :, n:] = -4.0 + 0.3 * torch.randn(80, T - n, generator=gen)
    return mel.to(DEV)


def _assert_equals_alone(g, mel, lens, wav):
    """every valid sample of the ragged batch's wav is bit-equal to the B = 1 call on the unpadded mel; exact zeros beyond"""
    assert tuple(wav.shape) == (mel.shape[0], 1, HOP * mel.shape[2])
    for b, n in enumerate(lens):
        n = min(n, mel.shape[2])
        if n > 0:
            alone = g(mel[b:b + 1, :, :n])
            assert tuple(alone.shape) == (1, 1, HOP * n)
            assert torch.isfinite(alone).all()
            assert torch.equal(wav[b, 0, :HOP * n], alone[0, 0]), (b, n, (wav[b, 0, :HOP * n] - alone[0, 0]).abs().max().item())
        assert (wav[b, 0, HOP * n:] == 0).all(), (b, n)


# 1 ------------------------------------------------------------------------------------------------------------------------------
def test_g20_each_utterance_matches_the_reference_alone(arith):
    g, _, _ = _small_generator()
    mel, lens, wavs = _g20()
    out = g(mel.to(DEV), lens=lens).cpu()
    assert tuple(out.shape) == (4, 1, HOP * 32) and not out.requires_grad
    for b, n in enumerate(lens):
        e = (out[b, 0, :HOP * n] - wavs[b]).abs().max().item()
        print(f"g20 utterance {b} ({n} frames): max abs vs the reference's B = 1 output {e:.3e}")
        assert e <= BAR, (b, e)
        assert (out[b, 0, HOP * n:] == 0).all()


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_is_bit_equal_to_per_utterance_calls_reduced(arith):
    g, _, _ = _small_generator()
    mel, lens, _ = _g20()
    mel = mel.to(DEV)
    _assert_equals_alone(g, mel, lens, g(mel, lens=lens))


def test_ragged_batch_is_bit_equal_to_per_utterance_calls_v1_canonical(arith):
    from ctts_amd.synthetic import make_batch
    lens = [int(v) for v in make_batch(seed=1234)["mel_lens"]]
    assert len(lens) == 16 and sum(lens) == 11992 and max(lens) == 1024
    g = _v1_generator()
    mel = _padded_mel(lens, 1024, 3)
    wav = g(mel, lens=lens)
    _assert_equals_alone(g, mel, lens, wav)


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_lengths_around_tile_and_halo_edges_v1(arith):
    lens = [1, 2, 15, 16, 17, 127, 128, 129]
    g = _v1_generator()
    mel = _padded_mel(lens, 131, 5)                          # T = 131: a multiple of neither the 128-row tile nor anything else
    _assert_equals_alone(g, mel, lens, g(mel, lens=lens))


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_padding_is_never_read(arith):
    g, _, _ = _small_generator()
    mel, lens, _ = _g20()
    mel = mel.to(DEV)
    clean = g(mel, lens=lens)
    assert torch.isfinite(clean).all()
    for fill in (float("nan"), float("inf"), 1e30, -3e38):
        dirty = mel.clone()
        for b, n in enumerate(lens):
            dirty[b, :, n:] = fill
        out = g(dirty, lens=lens)
        assert torch.isfinite(out).all(), fill
        assert torch.equal(out, clean), fill
    gv = _v1_generator()
    lv = [1, 17, 129, 40]
    melv = _padded_mel(lv, 131, 6)
    cleanv = gv(melv, lens=lv)
    for b, n in enumerate(lv):
        melv[b, :, n:] = float("nan")
    outv = gv(melv, lens=lv)
    assert torch.isfinite(outv).all() and torch.equal(outv, cleanv)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_full_lengths_equal_dense_and_no_state_left_behind(arith):
    g, _, _ = _small_generator()
    mel, lens, _ = _g20()
    mel = mel.to(DEV)
    dense = g(mel)
    assert torch.equal(g(mel, lens=[32] * 4), dense)
    assert torch.equal(g(mel, lens=None), dense)
    ragged = g(mel, lens=lens)
    assert not torch.equal(ragged, dense)
    assert torch.equal(g(mel), dense)                        # a dense call after a ragged one: as before it
    gv = _v1_generator()
    melv = _padded_mel([131, 131], 131, 7)
    dv = gv(melv)
    assert torch.equal(gv(melv, lens=torch.tensor([131, 131], device=DEV)), dv)
    gv(melv, lens=[5, 77])
    assert torch.equal(gv(melv), dv)


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_empty_and_overlong_utterances(arith):
    g, _, _ = _small_generator()
    mel, lens, _ = _g20()
    mel = mel.to(DEV)
    base = g(mel, lens=lens)
    out = g(mel, lens=[32, 0, 1, 27])
    assert (out[1] == 0).all()
    for b in (0, 2, 3):
        assert torch.equal(out[b], base[b])
    assert (g(mel, lens=[0, 0, 0, 0]) == 0).all()
    dense = g(mel)
    for big in (33, 1000, 2 ** 31 - 1):
        o32 = g(mel, lens=torch.tensor([big, 13, 1, 27], dtype=torch.int32, device=DEV))
        assert torch.equal(o32[0], dense[0]) and torch.equal(o32[1:], base[1:]), big
    o64 = g(mel, lens=torch.tensor([2 ** 40, 13, 1, 27], dtype=torch.int64, device=DEV))
    assert torch.equal(o64, o32)
    neg = g(mel, lens=torch.tensor([32, -5, 1, 27], dtype=torch.int32, device=DEV))      # a negative count is an empty utterance
    assert torch.equal(neg, out)


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_model_mel_view_and_int64_mel_lens_feed_the_ragged_vocoder(arith):
    from ctts_amd.configs import get_configs
    from ctts_amd.synthetic import make_batch, to_device, as_model_args
    pre, mc, tc = get_configs()
    torch.manual_seed(0)
    model = ctts_amd.CompTransTTS(pre, mc, tc).to(DEV).eval()
    args = as_model_args(to_device(make_batch([12, 9], 40, seed=4), DEV))
    with torch.no_grad():
        outs = model(*args[:4])
    mel, mel_lens = outs[1], outs[9]                         # postnet mel [B, T, 80] channel-last, predicted lengths int64 on the device
    assert mel.is_contiguous() and mel.shape[2] == 80 and mel_lens.is_cuda and mel_lens.dtype == torch.int64
    lens = mel_lens.tolist()
    print("predicted mel_lens", lens, "of", mel.shape[1])
    g, h, sd = _small_generator()
    view = mel.transpose(1, 2)                               # what utils/tools.py:342-350 hands vocoder_infer
    assert not view.is_contiguous() and view.data_ptr() == mel.data_ptr()
    a = g(view, lens=mel_lens)
    assert torch.equal(a, g(view.contiguous(), lens=mel_lens))
    assert torch.equal(a, g(view, lens=lens))
    _assert_equals_alone(g, view, lens, a)
    short = (mel_lens - 3 * torch.arange(1, len(lens) + 1, device=DEV)).clamp(min=1)      # still int64 on the device, surely ragged
    _assert_equals_alone(g, view, short.tolist(), g(view, lens=short))
    W = R.fold_state_dict(sd, dtype=torch.float64)
    for b, n in enumerate(lens):
        if n > 0:
            ref = R.generator_forward(W, h, view[b:b + 1, :, :n].double().cpu())[0, 0]
            assert (a[b, 0, :HOP * n].double().cpu() - ref).abs().max().item() <= BAR, b
    wavs = vocoder.infer_wavs(g, view, mel_lens, 32768.0)
    assert len(wavs) == len(lens)
    for b, n in enumerate(lens):
        assert wavs[b].dtype == np.int16 and wavs[b].shape == (HOP * n,)
        assert np.array_equal(wavs[b], (a[b, 0, :HOP * n].cpu().numpy() * 32768.0).astype("int16"))


# 8 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_captured_forward_replays_with_new_lengths(arith, dtype):
    g, _, _ = _small_generator()
    mel, lens, _ = _g20()
    mel = mel.to(DEV)
    static_lens = torch.tensor(lens, dtype=dtype, device=DEV)
    eager_first = g(mel, lens=static_lens)                   # warm-up: fills the packed-weight cache outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # one stream, no parallel branches
        captured = g(mel, lens=static_lens)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager_first)
    for new in ([5, 32, 20, 0], [1, 1, 32, 31]):
        static_lens.copy_(torch.tensor(new, dtype=dtype, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = captured.clone()
        want = g(mel, lens=torch.tensor(new, dtype=dtype, device=DEV))
        assert torch.equal(got, want), new
        for b, n in enumerate(new):
            assert (got[b, 0, HOP * n:] == 0).all()
