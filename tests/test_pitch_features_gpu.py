"""GPU: the pitch tracker and the F0 -> continuous log-F0 -> CWT target chain (csrc/pitchtrack.hip) through ctts_amd.pitch_features,
against the float64 restatements of tests/pitch_restate.py.

Tolerance rule (no figure here comes from the kernels): an output's largest error against float64 may be 3 x the largest error of the
float32 twin - the same restatement run on float32 arrays - on the same input; for f0 the error is relative and has a floor of 1e-5.
tests/test_pitch_restate_cpu.py::test_decision_margin shows that float32 arithmetic cannot flip a voicing or winner decision on these
inputs, so every frame is compared and voiced / unvoiced must agree on every frame.  Measured pairs are printed under -s."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402
from ctts_amd import _lib, kernels as K, pitch_features as PF  # noqa: E402
import pitch_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TWIN_X = 3.0
F0_REL_FLOOR = 1e-5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _check_tracker(name, f0, st, wav, lens):
    f64, s64 = R.track_pitch(wav, lens)
    f32, s32 = R.track_pitch(wav, lens, dtype=np.float32)
    f0, st = _np(f0), _np(st)
    assert f0.dtype == np.float32 and f0.shape == f64.shape and st.shape == s64.shape
    assert np.isfinite(f0).all() and np.isfinite(st).all()
    assert np.array_equal(f0 > 0, f64 > 0), f"{name}: voiced / unvoiced differs at {np.argwhere((f0 > 0) != (f64 > 0))}"
    assert np.array_equal(f32 > 0, f64 > 0)
    v = f64 > 0
    assert v.any()
    twin_f = (np.abs(f32.astype(np.float64) - f64)[v] / f64[v]).max()
    got_f = (np.abs(f0.astype(np.float64) - f64)[v] / f64[v]).max()
    twin_s = np.abs(s32.astype(np.float64) - s64).max()
    got_s = np.abs(st.astype(np.float64) - s64).max()
    print(f"{name}: f0 rel err {got_f:.3e} (twin {twin_f:.3e}), strength abs err {got_s:.3e} (twin {twin_s:.3e}), voiced {v.sum()} / {v.size}")
    assert got_f <= max(TWIN_X * twin_f, F0_REL_FLOOR)
    assert got_s <= TWIN_X * twin_s
    return f64


def test_tracker_ragged_batch_against_float64():
    wav = R.gpu_tracker_batch()
    lens = R.GPU_TRACK_LENS
    f0, st = PF.track_pitch(_dev(wav), _i32(lens))
    assert f0.shape == (3, 27)
    f64 = _check_tracker("ragged", f0, st, wav, lens)
    f0n, stn = _np(f0), _np(st)
    for b, n in enumerate(lens):
        fb = 1 + n // R.HOP
        assert not f0n[b, fb:].any() and not stn[b, fb:].any(), "frames beyond the length must be exactly 0"
    assert (f64[1, 2:8] > 0).all() and not f64[1, 13:20].any()          # utterance 1: tone, then noise
    # each utterance equals its own B = 1 call, bit for bit; two runs are bit-identical
    w = _dev(wav)
    for b, n in enumerate(lens):
        f1, s1 = PF.track_pitch(w[b:b + 1].contiguous(), _i32([n]))
        assert torch.equal(f1[0], f0[b]) and torch.equal(s1[0], st[b]), b
    f2, s2 = PF.track_pitch(w, _i32(lens))
    assert torch.equal(f2, f0) and torch.equal(s2, st)


def test_tracker_dense_and_silence():
    wav = R.gpu_tracker_batch()
    f0, st = PF.track_pitch(_dev(wav))                                    # lens = NULL: every utterance has N samples
    _check_tracker("dense", f0, st, wav, None)
    sil = R.gpu_silence_batch()
    f0, st = PF.track_pitch(_dev(sil))
    _check_tracker("silence+tone", f0, st, sil, None)
    assert not _np(f0)[0].any() and not _np(st)[0].any(), "digital silence is unvoiced with strength 0, never NaN"


def test_tracker_refuses_bad_arguments():
    w = torch.zeros(1, 2048, device=DEV)
    with pytest.raises(_lib.CttsError, match="does not fit the 1024-sample frame"):
        PF.track_pitch(w, f0_min=40.0)                                   # lags up to 552
    with pytest.raises(_lib.CttsError, match="does not fit the 1024-sample frame"):
        PF.track_pitch(w, f0_max=20000.0)
    with pytest.raises(_lib.CttsError):
        PF.track_pitch(torch.zeros(1, 2048))                             # CPU tensor
    with pytest.raises(_lib.CttsError):
        PF.track_pitch(w.double())
    with pytest.raises(_lib.CttsError):
        PF.track_pitch(w, torch.tensor([2048], dtype=torch.int32))       # CPU lengths
    with pytest.raises(_lib.CttsError):
        PF.track_pitch(torch.zeros(2, 2049, device=DEV)[:, 1:])          # not contiguous
    with pytest.raises(_lib.CttsError):
        K.pitch_track(w, PF.prepare(DEV), _i32([5, 5]))


def _check_chain(name, f0, frames):
    t = PF.f0_targets(_dev(f0), _i32(frames))
    r64 = R.f0_targets(f0, frames)
    r32 = R.f0_targets(f0, frames, dtype=np.float32)
    assert np.array_equal(_np(t["valid"]), r64["valid"]) and t["valid"].dtype == torch.int32
    assert np.array_equal(r32["valid"], r64["valid"])
    assert np.array_equal(_np(t["uv"]), r64["uv"].astype(np.float32))
    # one comparison per output array of ctts_f0_targets: cont_lf0 [B,F], mean_std [B,2], cwt_spec [B,F,10]
    def outputs(d, conv):
        return {"cont_lf0": conv(d["cont_lf0"]), "mean_std": np.stack([conv(d["f0_mean"]), conv(d["f0_std"])], 1), "cwt_spec": conv(d["cwt_spec"])}
    got_all, r64o, r32o = outputs(t, _np), outputs(r64, np.asarray), outputs(r32, np.asarray)
    for key in ("cont_lf0", "mean_std", "cwt_spec"):
        got = got_all[key]
        assert got.dtype == np.float32 and got.shape == r64o[key].shape and np.isfinite(got).all()
        e = np.abs(got.astype(np.float64) - r64o[key]).max()
        twin = np.abs(r32o[key].astype(np.float64) - r64o[key]).max()
        print(f"{name} {key}: abs err {e:.3e} (twin {twin:.3e}), max |ref| {np.abs(r64o[key]).max():.3g}")
        assert e <= TWIN_X * twin, key
    for b, n in enumerate(frames):
        for key in ("uv", "cont_lf0", "cwt_spec"):
            assert not _np(t[key])[b, n:].any(), "frames beyond the length must be exactly 0"
        if not r64["valid"][b]:
            for key in ("uv", "cont_lf0", "cwt_spec", "f0_mean", "f0_std"):
                assert not _np(t[key])[b].any(), f"invalid utterance {b}: {key} must be all zero"
    return t


def test_chain_against_float64_and_batch_independence():
    f0, frames = R.gpu_chain_batch(), R.CHAIN_FRAMES
    t = _check_chain("chain", f0, frames)
    assert _np(t["valid"]).tolist() == [1, 1, 1, 0]                       # one frame: constant contour
    d = _dev(f0)
    for b, n in enumerate(frames):                                        # its own B = 1 call: its own M = 64, 64, 8, 1
        t1 = PF.f0_targets(d[b:b + 1].contiguous(), _i32([n]))
        for key in ("uv", "cont_lf0", "cwt_spec", "f0_mean", "f0_std", "valid"):
            assert torch.equal(t1[key][0], t[key][b]), (b, key)
    t2 = PF.f0_targets(d, _i32(frames))
    for key in t:
        assert torch.equal(t2[key], t[key]), key


def test_chain_invalid_utterances():
    f0, frames = R.gpu_chain_invalid_batch()
    t = _check_chain("invalid", f0, frames)
    assert _np(t["valid"]).tolist() == [0, 0, 1]                          # all unvoiced; std == 0; a regular track
    bad = f0.copy()
    bad[2, 7] = -100.0                                                    # log of a negative value: non-finite -> dropped, zeros
    t = PF.f0_targets(_dev(bad), _i32(frames))
    assert _np(t["valid"]).tolist() == [0, 0, 0]
    for key in ("uv", "cont_lf0", "cwt_spec", "f0_mean", "f0_std"):
        assert not _np(t[key]).any() and np.isfinite(_np(t[key])).all()


def test_norm_interp_f0_against_float64():
    for f0, frames in ((R.gpu_chain_batch(), R.CHAIN_FRAMES), R.gpu_chain_invalid_batch()):
        y, uv = K.norm_interp_f0(_dev(f0), _i32(frames))
        y64, uv64 = R.norm_interp_f0_batch(f0, frames)
        y32, _ = R.norm_interp_f0_batch(f0, frames, dtype=np.float32)
        assert np.array_equal(_np(uv), uv64.astype(np.float32))
        e = np.abs(_np(y).astype(np.float64) - y64).max()
        twin = np.abs(y32.astype(np.float64) - y64).max()
        print(f"norm_interp_f0: abs err {e:.3e} (twin {twin:.3e})")
        assert e <= TWIN_X * twin
    assert not _np(y)[0].any(), "an all-unvoiced utterance gives zeros"


def test_chain_length_limit_and_cpu_tensors():
    rng = np.random.default_rng(3)
    f0 = (150.0 + 50.0 * rng.random((1, 4096))).astype(np.float32)
    f0[0, rng.random(4096) < 0.3] = 0
    t = _check_chain("n=4096", f0, (4096,))
    assert _np(t["valid"]).tolist() == [1]
    with pytest.raises(_lib.CttsError, match="at most 4096 frames"):
        PF.f0_targets(torch.zeros(1, 4097, device=DEV), _i32([4097]))
    with pytest.raises(_lib.CttsError, match="at most 4096 frames"):
        K.norm_interp_f0(torch.zeros(1, 4097, device=DEV), _i32([4097]))
    with pytest.raises(_lib.CttsError):
        PF.f0_targets(torch.zeros(1, 64), _i32([64]))
    with pytest.raises(_lib.CttsError):
        PF.f0_targets(torch.zeros(1, 64, device=DEV), torch.tensor([64], dtype=torch.int32))
    with pytest.raises(_lib.CttsError):
        PF.f0_targets(torch.zeros(1, 64, device=DEV, dtype=torch.float64), _i32([64]))
    with pytest.raises(_lib.CttsError):
        K.f0_targets(torch.zeros(2, 64, device=DEV), _i32([64]))


def test_pitch_targets_feed_the_model():
    from ctts_amd.configs import get_configs
    from ctts_amd.synthetic import make_batch, to_device, as_model_args

    lens = R.GPU_TRACK_LENS
    wav = _dev(R.gpu_tracker_batch()[:, :max(lens)])                      # padded to the longest utterance, like a collated batch
    pre, mc, tc = get_configs()
    stft = ctts_amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(DEV)
    batch = to_device(make_batch([13, 10, 3], 2, seed=5), DEV)            # mel lengths 26, 20, 6 = 1 + lens // 256
    assert batch["mel_lens"].tolist() == [1 + n // 256 for n in lens]
    mel2ph = batch["p_targets"]["mel2ph"]
    p = PF.pitch_targets_from_wav(wav, _i32(lens), stft, mel2ph=mel2ph)
    Tm = 26
    assert set(p) >= {"f0", "uv", "cwt_spec", "f0_mean", "f0_std", "mel2ph", "valid"}
    assert p["f0"].shape == (3, Tm) and p["uv"].shape == (3, Tm) and p["cwt_spec"].shape == (3, Tm, 10)
    assert p["f0_mean"].shape == (3,) and p["f0_std"].shape == (3,) and p["valid"].shape == (3,)
    for k in ("f0", "uv", "cwt_spec", "f0_mean", "f0_std"):
        assert p[k].dtype == torch.float32 and p[k].is_cuda and torch.isfinite(p[k]).all(), k
    assert p["mel2ph"] is mel2ph and p["valid"].tolist() == [1, 1, 1]
    batch["p_targets"] = p
    torch.manual_seed(0)
    model = ctts_amd.CompTransTTS(pre, mc, tc).to(DEV)
    model.train()
    out = model(*as_model_args(batch))
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()
    assert out[0].shape[:2] == (3, Tm)
