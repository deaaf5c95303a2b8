"""CPU: pins tests/speaker_restate.py, the float64 statement of the DeepSpeaker embedding the kernels of csrc/speaker.hip are tested
against, the fairness of the shared inputs, and the host side of ctts_amd.speaker (weights in and out, refusals, the ABI names)."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctts_amd
from ctts_amd import _lib
from ctts_amd import speaker as S
from tests import speaker_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_percentile_equals_numpy_on_float64_copies():
    rng = np.random.default_rng(0)
    sizes = list(range(1, 260)) + [1000, 1001, 4001, 30011]
    for n in sizes:
        for a in (np.abs(rng.standard_normal(n)).astype(np.float32), rng.integers(0, 3, n).astype(np.float32)):     # the second: ties
            assert R.percentile95(a) == float(np.percentile(a.astype(np.float64), 95)), n
    for name, x in R.span_cases().items():
        a = np.abs(x)
        assert R.percentile95(a) == float(np.percentile(a.astype(np.float64), 95)), name


def test_span_of_the_designed_inputs():
    assert R.span(np.zeros(100, np.float32)) == (0, 0, 0)
    c = R.span_cases()
    assert R.span(c["one_loud"]) == (1234, 1234, 0) and R.span(c["len1"]) == (0, 0, 0)
    assert R.span(c["square"])[2] == 0                                   # half the samples tie at the largest level: none exceeds it
    assert R.span(c["square_step"]) == (1000, 1099, 1)
    assert R.span(c["ramp41"]) == (39, 40, 1)                            # v = 38: thr = a[38] exactly, two samples above
    for name, x in R.fbank_cases().items():
        L = 9000 if name == "zeros_inside" else int(name[1:])
        assert R.span(x) == (137, 137 + L, 1), name
    for name, x, nf, _ in R.crop_cases():
        first, last, valid = R.span(x)
        assert valid and R.n_frames(last - first) == nf, name


def test_frame_counts_and_filterbank_bins():
    assert [R.n_frames(L) for L in (551, 552, 772, 773, 35690, 35911)] == [1, 2, 2, 3, 160, 161]
    assert [S.n_frames_of(L) for L in (0, 1, 551, 552, 772, 773, 35690, 35911)] == [0, 1, 1, 2, 2, 3, 160, 161]
    assert round(0.025 * R.SR + 1e-9) == R.FRAME and int(np.floor(0.01 * R.SR + 0.5)) == R.STEP      # round-half-up of 551.25 and 220.5
    b = R.bins()
    assert b[:12].tolist() == [0, 1, 2, 4, 6, 7, 9, 11, 13, 15, 17, 19] and b[-3:].tolist() == [467, 489, 512]
    assert len(b) == 66 and len(set(b.tolist())) == 66
    assert S.fbank_bins().tolist() == b.tolist()
    fb = R.filterbank()
    assert fb.shape == (64, 513) and fb.min() >= 0 and fb.max() == 1.0 and (fb[:, 512] == 0).all()
    assert (fb.argmax(1) == b[1:-1]).all()


def test_zero_frames_normalise_to_zero_and_no_logarithm():
    x = R.fbank_cases()["zeros_inside"]
    fb = R.fbank(x[137:137 + 9000])
    zero_rows = [i for i in range(fb.shape[0]) if i * R.STEP > 3000 and i * R.STEP + R.FRAME <= 5000]
    assert len(zero_rows) >= 3 and all((fb[i] == 0).all() for i in zero_rows)
    nz = fb[0]
    assert abs(float(nz.mean())) < 1e-12 and abs(float(nz.std(unbiased=False)) - 1) < 1e-12


@pytest.mark.parametrize("H,W", [(8, 6), (7, 5), (10, 4), (1, 1)])
def test_conv_equals_conv2d_on_the_explicitly_padded_input(H, W):
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.randn(2, H, W, 3, generator=g, dtype=torch.float64)
    for k, s in ((5, 2), (3, 1)):
        w = torch.randn(k, k, 3, 4, generator=g, dtype=torch.float64)
        pads = {(5, 2): ((1, 2) if H % 2 == 0 else (2, 2), (1, 2) if W % 2 == 0 else (2, 2)), (3, 1): ((1, 1), (1, 1))}[(k, s)]
        assert R.same_pads(H, k, s)[1:] == pads[0] and R.same_pads(W, k, s)[1:] == pads[1]
        xp = F.pad(x.permute(0, 3, 1, 2), (pads[1][0], pads[1][1], pads[0][0], pads[0][1]))
        want = F.conv2d(xp, w.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)
        got = R.conv_nhwc(x, w, s)
        assert got.shape == (2, -(-H // s), -(-W // s), 4) and float((got - want).abs().max()) < 1e-12


def test_stage_shapes_and_clip_shares_on_the_gpu_inputs():
    ref = R.net_reference()["f64"]
    assert [tuple(s.shape[1:]) for s in ref["stages"]] == [(80, 32, 64), (40, 16, 128), (20, 8, 256), (10, 4, 512)]
    assert ref["valid"] == [1, 1, 0] and ref["n_frames"][0] > 160 > ref["n_frames"][1] > 0
    assert len(ref["clipped"]) == 40
    at_top = []
    for i, y in enumerate(ref["clipped"]):
        inside = float(((y > 0) & (y < 20)).double().mean())
        assert inside >= 0.10, (i, inside)
        at_top.append(float((y == 20).double().mean()))
    assert max(at_top) >= 0.01, at_top
    assert (ref["embedding"][2] == 0).all() and abs(float(ref["embedding"][0].norm()) - 1) < 1e-12


def test_wrong_readings_differ_by_more_than_the_gpu_bar():
    ref = R.net_reference()
    x = R.net_batch()[0]
    right, twin = ref["f64"]["fbank"][0], ref["f32"]["fbank"][0].double()
    bar = 4 * float((twin - right).abs().max())
    for wrong in ({"log": True}, {"hann": True}, {"sample_std": True}):
        fb = R.features(x, **wrong)[0]
        assert float((fb - right).abs().max()) > bar, (wrong, bar)
    # one more sample at the end of the span shows in the last frame, which the centre crop of the long utterance drops: the short one
    short, twin1 = ref["f64"]["fbank"][1], ref["f32"]["fbank"][1].double()
    fb = R.features(R.net_batch()[1], include_last=True)[0]
    assert float((fb - short).abs().max()) > 4 * float((twin1 - short).abs().max())
    # the net: on the first utterance alone (a row does not depend on the others)
    w = R.make_weights()
    emb_bar = 4 * float((ref["f32"]["embedding"][0].double() - ref["f64"]["embedding"][0]).abs().max())
    stage_bar = [4 * float((a[0].double() - b[0]).abs().max()) for a, b in zip(ref["f32"]["stages"], ref["f64"]["stages"])]
    for wrong in ({"wrong_even": True}, {"bn_eps": 1e-5}):
        emb, stages, _ = R.rescnn(w, right[None], **wrong)
        for s, want, b in zip(stages, ref["f64"]["stages"], stage_bar):
            assert float((s[0] - want[0]).abs().max()) > b, wrong
        assert float((emb[0] - ref["f64"]["embedding"][0]).abs().max()) > emb_bar, wrong
    # the feature order changes nothing before the Reshape
    x4 = ref["f64"]["stages"][3][:1]
    W = {k: torch.as_tensor(v).double() for k, v in w.items()}
    z = x4.permute(0, 1, 3, 2).reshape(1, 10, -1).mean(1) @ W["affine/kernel"] + W["affine/bias"]
    emb = z / z.norm(dim=1, keepdim=True)
    assert float((emb[0] - ref["f64"]["embedding"][0]).abs().max()) > emb_bar


def test_weights_round_trip_and_refusals(tmp_path):
    w = R.make_weights()
    assert set(w) == set(S.weight_shapes()) and len(w) == 28 * 6 + 2
    e = S.DeepSpeakerEmbedder(w)
    path = str(tmp_path / "w.npz")
    e.save_npz(path)
    e2 = S.DeepSpeakerEmbedder.from_npz(path)
    assert set(e2.weights) == set(w) and all(np.array_equal(e2.weights[k], w[k]) and e2.weights[k].dtype == np.float32 for k in w)
    missing = dict(w)
    del missing["res3_1_branch_2b_bn/moving_variance"]
    with pytest.raises(ctts_amd._lib.CttsError, match="res3_1_branch_2b_bn/moving_variance"):
        S.DeepSpeakerEmbedder(missing)
    with pytest.raises(ctts_amd._lib.CttsError, match="softmax/kernel"):
        S.DeepSpeakerEmbedder(dict(w, **{"softmax/kernel": np.zeros((512, 10), np.float32)}))
    with pytest.raises(ctts_amd._lib.CttsError, match="conv128-s/kernel"):
        S.DeepSpeakerEmbedder(dict(w, **{"conv128-s/kernel": np.zeros((5, 5, 128, 64), np.float32)}))
    with pytest.raises(ctts_amd._lib.CttsError, match="22050"):
        S.DeepSpeakerEmbedder(w, sampling_rate=16000)


def test_batchnorm_fold_is_the_unfolded_layer():
    rng = np.random.default_rng(1)
    k, b = rng.standard_normal((3, 3, 4, 5)), rng.standard_normal(5)
    g, be, m, v = rng.uniform(0.5, 1.5, 5), rng.standard_normal(5), rng.standard_normal(5), rng.uniform(0.5, 1.5, 5)
    wk, wb = S.fold_batchnorm(k, b, g, be, m, v)
    x = torch.randn(1, 6, 6, 4, dtype=torch.float64)
    want = (R.conv_nhwc(x, torch.as_tensor(k), 1) + torch.as_tensor(b) - torch.as_tensor(m)) / torch.sqrt(torch.as_tensor(v) + 1e-3) * torch.as_tensor(g) + torch.as_tensor(be)
    got = R.conv_nhwc(x, torch.as_tensor(wk), 1) + torch.as_tensor(wb)
    assert float((got - want).abs().max()) < 1e-12


def test_from_h5_without_h5py_raises_import_error(monkeypatch, tmp_path):
    monkeypatch.setitem(sys.modules, "h5py", None)          # `import h5py` raises ImportError, installed or not
    with pytest.raises(ImportError, match="h5py"):
        S.DeepSpeakerEmbedder.from_h5(str(tmp_path / "ResCNN_triplet_training_checkpoint_265.h5"))


def test_cpu_tensors_are_refused():
    e = S.DeepSpeakerEmbedder(R.make_weights())
    wav = torch.zeros(2, 4000)
    for call in (lambda: e(wav, [4000, 3000]), lambda: e.features(wav, [4000, 3000]), lambda: e.forward_features(torch.zeros(1, 160, 64)),
                 lambda: e.to("cpu"), lambda: ctts_amd.metrics.speaker_similarity(wav, None, wav, None, e),
                 lambda: ctts_amd.preprocess.speaker_embeddings([wav[0]], ["p225"], e)):
        with pytest.raises(ctts_amd._lib.CttsError):
            call()
    assert ctts_amd.DeepSpeakerEmbedder is S.DeepSpeakerEmbedder and ctts_amd.speaker_similarity is ctts_amd.metrics.speaker_similarity


def test_abi_names_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ctts.h")).read()
    declared = set(re.findall(r"\b(ctts_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ctts_speaker_frames", "ctts_speaker_span", "ctts_speaker_fbank", "ctts_conv2d_nhwc", "ctts_conv2d_nhwc_workspace_bytes",
                 "ctts_speaker_head"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
