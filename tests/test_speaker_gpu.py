"""GPU: the speaker-embedding kernels (csrc/speaker.hip through the C ABI, ctts_amd.kernels and ctts_amd.speaker) against the float64
restatement of tests/speaker_restate.py (itself pinned in tests/test_speaker_restate_cpu.py).

Bars - nothing is taken from the code under test.  The span is exact.  Every float comparison prints (with -s) the kernel's largest
error against float64, the float32 twin's on the same input, and the bar = 4 x the twin's: two correct fp32 implementations with
different butterfly and accumulation orders differ from each other by about what each differs from float64.  The convolution unit
cases use the K-dependent bound tests/gemm_cases.product_bound applies to the same arithmetic (the fp32 MFMA tile kernels):
2e-6 max(1, K / 16) max(1, |pre-activation|max); clipping is 1-Lipschitz, so the bound holds for the clipped output too.  No element
or frame is excluded from any comparison; outputs are compared as whole buffers with guard cells.

Measured on the MI355X (kernel / twin max-abs error against float64):
  fbank and crop cases: kernel at most 2.4e-7 (crop F270), at most 0.32 of the twin's error (L552: 1.2e-7 / 3.7e-7)
  whole net: fbank 2.3e-7 / 3.1e-6; stage 1..4 4.7e-5 / 4.1e-5, 2.1e-4 / 2.5e-4, 3.3e-4 / 3.5e-4, 3.5e-4 / 5.1e-4 (values up to 20,
  a clip away from saturation amplifies one rounding); embedding 1.6e-7 / 1.9e-7; similarity 0.99645019 against 0.99645019 (bar 3.4e-5)
  126 conv unit cases: largest error / bound 0.031; K = 4608 (split 8 ways): 5.3e-6 and 6.4e-6 against bounds of 6.9e-3 and 6.6e-3,
  the twin 1.2e-5 and 1.0e-5"""
import ctypes

import numpy as np
import pytest
import torch

import ctts_amd
from ctts_amd import _lib
from ctts_amd import kernels as K
from ctts_amd import speaker as S
from tests import speaker_restate as R
from tests.gemm_cases import product_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


def guarded(shape, dtype=torch.float32, fill=-777.0):
    """a device buffer with GUARD cells of `fill` on both sides of a view of `shape`"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, fill=-777.0):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def batch_of(sigs, beyond=0.0):
    """[B, N] device batch; cells at and beyond a row's length hold `beyond`"""
    lens = [len(s) for s in sigs]
    host = np.full((len(sigs), max(lens) + 3), beyond, np.float32)
    for i, s in enumerate(sigs):
        host[i, :lens[i]] = s
    return torch.from_numpy(host).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), lens


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def embedder():
    return S.DeepSpeakerEmbedder(R.make_weights(), DEV)


# ---- span ------------------------------------------------------------------------------------------------------------------------------
def test_span_is_exact_on_a_ragged_batch():
    cases = R.span_cases()
    names = list(cases)
    wav, lens_d, lens = batch_of([cases[n] for n in names], beyond=5.0)          # ignoring lens would find the 5.0s
    B = len(names)
    bufs = [guarded((B,), torch.int32, -777) for _ in range(4)]
    lib = _lib.load()
    assert lib.ctts_speaker_span(wav.data_ptr(), lens_d.data_ptr(), *[v.data_ptr() for _, v in bufs], B, wav.shape[1], stream()) == 0
    first, last, frames, valid = (v.cpu().tolist() for _, v in bufs)
    assert all(guards_intact(b, -777) for b, _ in bufs)
    for i, n in enumerate(names):
        want = R.span(cases[n])
        assert (first[i], last[i], valid[i]) == want, (n, first[i], last[i], valid[i], want)
        assert frames[i] == (R.n_frames(want[1] - want[0]) if want[2] else 0), n
    assert valid[names.index("zeros")] == 0 and valid[names.index("one_loud")] == 0 and valid[names.index("len1")] == 0
    again = K.speaker_span(wav, lens_d)
    assert [t.cpu().tolist() for t in again] == [first, last, frames, valid]
    assert [K.speaker_frames(L) for L in (0, 1, 551, 552, 772, 773, 35690, 35911)] == [0, 1, 1, 2, 2, 3, 160, 161]


# ---- fbank -----------------------------------------------------------------------------------------------------------------------------
def _report(name, got, want, twin):
    err = float((got.double().cpu() - want).abs().max())
    terr = float((twin.double() - want).abs().max())
    print(f"SPEAKER {name}: kernel {err:.3e} twin {terr:.3e} bar {4 * terr:.3e}")
    assert err <= 4 * terr, f"{name}: max |err| {err:.3e} above 4 x the float32 twin's {terr:.3e}"
    return err


def test_fbank_frame_edges_and_zero_frames_vs_float64():
    cases = R.fbank_cases()
    names = list(cases)
    wav, lens_d, lens = batch_of([cases[n] for n in names])
    B, N = wav.shape
    first, last, frames, valid = K.speaker_span(wav, lens_d)
    OF = S.n_frames_of(N)
    bins = torch.from_numpy(S.fbank_bins()).to(DEV)
    buf, out = guarded((B, OF, 64))
    assert _lib.load().ctts_speaker_fbank(wav.data_ptr(), first.data_ptr(), last.data_ptr(), valid.data_ptr(), bins.data_ptr(), None,
                                          out.data_ptr(), B, N, OF, 0, stream()) == 0
    assert guards_intact(buf)
    for i, n in enumerate(names):
        f, l, v = R.span(cases[n])
        want, twin = R.fbank(cases[n][f:l]), R.fbank(cases[n][f:l], torch.float32)
        nf = want.shape[0]
        assert int(frames[i]) == nf and nf == {"L551": 1, "L552": 2, "L773": 3}.get(n, nf)
        _report(f"fbank {n} ({nf} frames)", out[i, :nf], want, twin)
        assert bool((out[i, nf:] == 0).all()), n
        if n == "zeros_inside":
            rows = [r for r in range(nf) if bool((want[r] == 0).all())]
            assert len(rows) >= 3 and bool((out[i, rows] == 0).all())
    e = S.DeepSpeakerEmbedder(R.make_weights(), DEV).features(wav, lens_d)
    assert torch.equal(e["fbank"], out) and torch.equal(e["n_frames"], frames)


def test_crop_and_pad_offsets():
    for name, x, nf, offs in R.crop_cases():
        wav, lens_d, _ = batch_of([x] * len(offs))
        B, N = wav.shape
        first, last, frames, valid = K.speaker_span(wav, lens_d)
        assert frames.cpu().tolist() == [nf] * B
        f, l, _ = R.span(x)
        full, twin = R.fbank(x[f:l]), R.fbank(x[f:l], torch.float32)
        bins = torch.from_numpy(S.fbank_bins()).to(DEV)
        buf, out = guarded((B, 160, 64))
        od = torch.tensor(offs, dtype=torch.int32, device=DEV)
        assert _lib.load().ctts_speaker_fbank(wav.data_ptr(), first.data_ptr(), last.data_ptr(), valid.data_ptr(), bins.data_ptr(),
                                              od.data_ptr(), out.data_ptr(), B, N, 160, 0, stream()) == 0
        assert guards_intact(buf)
        for i, r in enumerate(offs):
            _report(f"crop {name} r={r}", out[i], R.crop_pad(full, r), R.crop_pad(twin, r))
        centre = K.speaker_fbank(wav[:1], first[:1], last[:1], valid[:1], bins, 160, centre=True)
        assert torch.equal(centre[0], out[offs.index(max(nf - 160, 0) // 2)])
    e = S.DeepSpeakerEmbedder(R.make_weights(), DEV)
    with pytest.raises(_lib.CttsError, match="frame_offset"):
        e(wav, lens_d, frame_offset=[0] * (B - 1) + [nf - 160 + 1])


# ---- convolution through the C ABI -----------------------------------------------------------------------------------------------------
def _conv_case(B, H, W, Cin, Cout, geom, mode, seed, lo=-0.5, hi=0.75):
    g = torch.Generator().manual_seed(seed)
    k, s = (5, 2) if geom == 0 else (3, 1)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(k, k, Cin, Cout, generator=g) * (1.5 / np.sqrt(k * k * Cin / 4.0))
    bias = torch.randn(Cout, generator=g) * 0.3
    pre = R.conv_nhwc(x.double(), w.double(), s) + bias.double()
    res = torch.randn(pre.shape, generator=g) * 0.5
    want = pre.clamp(lo, hi)
    if mode:
        want = (want + res.double()).clamp(lo, hi)
    lib = _lib.load()
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), bias.to(DEV), res.to(DEV)
    nbytes = lib.ctts_conv2d_nhwc_workspace_bytes(B, H, W, Cin, Cout, geom)
    wsb, ws = guarded((max(nbytes // 4, 4),))
    buf, out = guarded(tuple(pre.shape))
    st = lib.ctts_conv2d_nhwc(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr() if mode else None, out.data_ptr(), B, H, W, Cin, Cout,
                              geom, mode, lo, hi, ws.data_ptr() if nbytes else None, stream())
    assert st == 0, lib.ctts_last_error()
    assert guards_intact(buf) and guards_intact(wsb)
    bound = product_bound("buf64", k * k * Cin)(float(pre.abs().max()))
    err = float((out.double().cpu() - want).abs().max())
    twin = R.conv_twin(x, w, s) + bias
    twin = twin.clamp(lo, hi) if not mode else (twin.clamp(lo, hi) + res).clamp(lo, hi)
    terr = float((twin.double() - want).abs().max())
    name = f"conv B{B} {H}x{W} Cin{Cin} Cout{Cout} geom{geom} mode{mode} split-ws {nbytes}"
    print(f"SPEAKER {name}: kernel {err:.3e} twin {terr:.3e} bound {bound:.3e}")
    assert err <= bound, f"{name}: max |err| {err:.3e} above the bound {bound:.3e}"
    via = K.conv2d_nhwc(xd, wd, bd, geom, lo, hi, res=rd if mode else None)
    assert torch.equal(via, out)
    return bool((want == lo).any()), bool((want == hi).any()), err / bound


@pytest.mark.parametrize("geom", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_conv2d_nhwc_smallest_shapes_vs_float64(geom, mode):
    at_lo = at_hi = False
    worst, seed = 0.0, 100 * geom + 10 * mode
    for H, W in ((1, 1), (7, 5), (8, 6), (10, 4)):
        for Cin in (1, 64):
            for Cout in (64, 128):
                for B in (1, 3):
                    seed += 1
                    a, b, r = _conv_case(B, H, W, Cin, Cout, geom, mode, seed)
                    at_lo, at_hi, worst = at_lo or a, at_hi or b, max(worst, r)
    assert at_lo and at_hi                       # both clip bounds bind
    print(f"SPEAKER conv geom{geom} mode{mode}: largest error / bound {worst:.3f}")


def test_conv2d_nhwc_long_k_is_split_and_exact_to_the_bound():
    assert _lib.load().ctts_conv2d_nhwc_workspace_bytes(1, 10, 4, 512, 512, 1) > 0          # K = 4608, 8 tiles: split
    for mode in (0, 1):
        a, b, _ = _conv_case(1, 10, 4, 512, 512, 1, mode, 900 + mode)
        assert a and b
    a, b, _ = _conv_case(2, 20, 8, 128, 256, 0, 1, 902)                                     # the strided geometry with K = 3200
    assert a and b


def test_conv2d_nhwc_refuses_what_it_cannot_do():
    x = torch.zeros(1, 4, 4, 32, device=DEV)
    with pytest.raises(_lib.CttsError):
        K.conv2d_nhwc(x, torch.zeros(3, 3, 32, 64, device=DEV), torch.zeros(64, device=DEV), K.CONV_K3S1, 0, 20)
    with pytest.raises(_lib.CttsError):
        K.conv2d_nhwc(torch.zeros(1, 4, 4, 64, device=DEV), torch.zeros(3, 3, 64, 96, device=DEV), torch.zeros(96, device=DEV), K.CONV_K3S1, 0, 20)
    with pytest.raises(_lib.CttsError):
        K.conv2d_nhwc(torch.zeros(1, 4, 4, 64), torch.zeros(3, 3, 64, 64), torch.zeros(64), K.CONV_K3S1, 0, 20)


# ---- the whole net ---------------------------------------------------------------------------------------------------------------------
def test_whole_net_stages_and_embedding_vs_float64(embedder):
    ref = R.net_reference()
    f64, f32 = ref["f64"], ref["f32"]
    wav, lens_d, lens = batch_of(R.net_batch(), beyond=3.0)
    res = embedder(wav, lens_d)
    for key in ("first", "last", "n_frames", "valid"):
        assert res[key].cpu().tolist() == f64[key], key
    fb = K.speaker_fbank(wav, res["first"], res["last"], res["valid"], embedder._bins, 160, centre=True)
    _report("net fbank", fb, f64["fbank"], f32["fbank"])
    emb, stages = embedder.forward_features(fb, return_stages=True, valid=res["valid"])
    for i, s in enumerate(stages):
        assert tuple(s.shape) == tuple(f64["stages"][i].shape)
        _report(f"net stage {i + 1}", s, f64["stages"][i], f32["stages"][i])
    _report("net embedding", emb, f64["embedding"], f32["embedding"])
    assert torch.equal(emb, res["embedding"]) and bool((emb[2] == 0).all())
    # bit-identical run to run
    res2 = embedder(wav, lens_d)
    emb2, stages2 = embedder.forward_features(fb, return_stages=True, valid=res["valid"])
    assert torch.equal(res2["embedding"], res["embedding"]) and torch.equal(emb2, emb)
    assert all(torch.equal(a, b) for a, b in zip(stages, stages2))
    # a row does not depend on the batch around it
    alone = embedder(wav[1:2], lens_d[1:2])
    assert torch.equal(alone["embedding"][0], res["embedding"][1])


def test_speaker_similarity_and_per_speaker_means(embedder):
    ref = R.net_reference()
    f64, f32 = ref["f64"]["embedding"], ref["f32"]["embedding"].double()
    a, b = R.net_batch()[:2]
    wa, la, _ = batch_of([a, b])
    wb, lb, _ = batch_of([a, a])
    sim = ctts_amd.speaker_similarity(wa, la, wb, lb, embedder).cpu().double()
    want = torch.stack([(f64[0] * f64[0]).sum(), (f64[1] * f64[0]).sum()])
    # |cos - cos'| <= ||da|| + ||db|| for unit vectors; each ||d|| <= sqrt(512) x the embedding bar (4 x the twin's max-abs error)
    bar = 2 * np.sqrt(512.0) * 4 * float((f32 - f64).abs().max()) + 2.0 ** -23
    print(f"SPEAKER similarity: got {sim.tolist()} want {want.tolist()} bar {bar:.3e}")
    assert abs(float(sim[0]) - 1.0) <= 2.0 ** -22 and float((sim - want).abs().max()) <= bar
    wavs = [torch.from_numpy(x).to(DEV) for x in R.net_batch()]
    per_utt, per_spk = ctts_amd.speaker_embeddings(wavs, ["p225", "p226", "p226"], embedder)
    assert per_utt["valid"].tolist() == [1, 1, 0] and set(per_spk) == {"p225", "p226"}
    assert np.array_equal(per_spk["p226"], per_utt["embedding"][1]) and np.array_equal(per_spk["p225"], per_utt["embedding"][0])
    assert float(np.abs(per_utt["embedding"].astype(np.float64) - ref["f64"]["embedding"].numpy()).max()) <= 4 * float((f32 - f64).abs().max())
