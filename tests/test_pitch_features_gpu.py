"""GPU: the pitch tracker and the F0 -> continuous log-F0 -> CWT target chain (csrc/pitchtrack.hip) through ctts_amd.pitch_features,
against the float64 restatements of tests/pitch_restate.py.

Tolerance rule (no figure here comes from the kernels): an output's largest error against float64 may be 3 x the largest error of the
float32 twin - the same restatement run on float32 arrays - on the same input; for f0 the error is relative and has a floor of 1e-5.
tests/test_pitch_restate_cpu.py::test_decision_margin shows that float32 arithmetic cannot flip a voicing or winner decision on these
inputs, so every frame is compared and voiced / unvoiced must agree on every frame.  Measured pairs are printed under -s.
On the stationary tones the device's f0 is also held to the TRUE frequency, within 2 x the float64 restatement's worst error
(R.TRACKER_TONES_WORST_REL_ERR, measured on the CPU)."""
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


def _check_tracker(name, f0, st, wav, lens, ref=None, expect_voiced=True, **params):
    """ref: (f0_64, strength_64, f0_32, strength_32) of the restatement where a fixture has computed them already"""
    f64, s64, f32, s32 = ref if ref is not None else R.track_pitch(wav, lens, **params) + R.track_pitch(wav, lens, dtype=np.float32, **params)
    f0, st = _np(f0), _np(st)
    assert f0.dtype == np.float32 and f0.shape == f64.shape and st.shape == s64.shape
    assert np.isfinite(f0).all() and np.isfinite(st).all()
    assert np.array_equal(f0 > 0, f64 > 0), f"{name}: voiced / unvoiced differs at {np.argwhere((f0 > 0) != (f64 > 0))}"
    assert np.array_equal(f32 > 0, f64 > 0)
    v = f64 > 0
    assert v.any() == expect_voiced
    twin_f = (np.abs(f32.astype(np.float64) - f64)[v] / f64[v]).max() if v.any() else 0.0
    got_f = (np.abs(f0.astype(np.float64) - f64)[v] / f64[v]).max() if v.any() else 0.0
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


# ------------------------------------------------------------------------------------------------------------------ lag range, rates, thresholds
# The cases of R.gpu_tracker_cases(): tests/test_pitch_restate_cpu.py holds each of them to the decision margins (test_decision_margin)
# and shows what each is for (test_cases_reach_the_lag_range_they_claim, test_threshold_cases, test_ragged_case_lengths).
@pytest.fixture(scope="module")
def cases():
    """R.gpu_tracker_cases() with `ref` = (f0_64, strength_64, f0_32, strength_32) of the restatement, computed once"""
    out = R.gpu_tracker_cases()
    for c in out.values():
        c["ref"] = R.track_pitch(c["wav"], c["lens"], **c["params"]) + R.track_pitch(c["wav"], c["lens"], dtype=np.float32, **c["params"])
    return out


def _run_case(c):
    return PF.track_pitch(_dev(c["wav"]), None if c["lens"] is None else _i32(c["lens"]), **c["params"])


@pytest.mark.parametrize("name", ["ground_truth", "edges", "ragged", "ragged_sr16k", "sr16k", "sr48k", "f0min50"])
def test_tracker_cases_against_float64(cases, name):
    c = cases[name]
    wav, lens, hop = c["wav"], c["lens"], c["params"].get("hop", R.HOP)
    B, N = wav.shape
    f0, st = _run_case(c)
    assert f0.shape == (B, 1 + N // hop) and st.shape == f0.shape
    f64 = _check_tracker(name, f0, st, wav, lens, ref=c["ref"], **c["params"])
    f0n, stn = _np(f0), _np(st)
    for b in range(B):
        n = R.case_length(c, b)
        fb = 1 + n // hop
        assert not f0n[b, fb:].any() and not stn[b, fb:].any(), "frames beyond 1 + len // hop must be exactly 0"
        if c["truth"][b] is not None:                                     # a stationary tone: the device against the TRUE frequency
            sel, hz = R.full_window_frames(n, hop), c["truth"][b]
            rel = (np.abs(f0n[b, sel].astype(np.float64) - hz) / hz).max()
            rel64 = (np.abs(f64[b, sel] - hz) / hz).max()
            print(f"{name}[{b}] {hz:g} Hz: f0 rel err to the true frequency {rel:.3e} (float64 restatement {rel64:.3e}) over {len(sel)} frames")
            assert (f0n[b, sel] > 0).all() and rel <= 2.0 * R.TRACKER_TONES_WORST_REL_ERR
    # each utterance equals its own B = 1 call, bit for bit (other workgroup, other wave, other position among the wave's four frames)
    w = _dev(wav)
    for b in range(B):
        f1, s1 = PF.track_pitch(w[b:b + 1].contiguous(), None if lens is None else _i32([lens[b]]), **c["params"])
        assert torch.equal(f1[0], f0[b]) and torch.equal(s1[0], st[b]), b


def test_octave_cost_decides_on_device(cases):
    """440 Hz (lags 50, 100, 150) and 700 Hz (31.5, 63, 94.5, ...): the sub-multiples are candidates of almost the fundamental's height in
    other registers and lanes of the wave; the restatement without the octave cost falls to one at 700 Hz (and the CPU test shows the
    heights are within 0.0025), so a device argmax that kept the fundamental did so by the cost"""
    c = cases["ground_truth"]
    f0 = _np(_run_case(c)[0])
    sel = R.full_window_frames(R.GROUND_TRUTH_N)
    plain, _ = R.track_pitch(c["wav"][4:5], use_octave_cost=False)
    assert (np.abs(plain[0, sel] - 700.0) / 700.0 > 0.3).all()
    for b, hz in ((3, 440.0), (4, 700.0)):
        rel = np.abs(f0[b, sel].astype(np.float64) - hz) / hz
        print(f"octave cost {hz:g} Hz: f0 rel err to the true frequency {rel.max():.3e}")
        assert rel.max() <= 2.0 * R.TRACKER_TONES_WORST_REL_ERR
    assert not f0[6].any() and not f0[7].any()                            # noise, silence


def test_thresholds_on_device(cases):
    """silence_threshold 0.03 / 0.01 and voicing_threshold 0.6 / 0.4: the decisions change as in the restatement, the strength does not
    change by a bit, and the silence peak is the utterance's own"""
    got = {}
    for name in ("silence_default", "silence_low", "voicing_default", "voicing_low"):
        c = cases[name]
        f0, st = _run_case(c)
        _check_tracker(name, f0, st, c["wav"], c["lens"], ref=c["ref"], expect_voiced=name != "voicing_default", **c["params"])
        got[name] = (f0, st)
    assert torch.equal(got["silence_default"][1], got["silence_low"][1]) and torch.equal(got["voicing_default"][1], got["voicing_low"][1])
    f_def, f_low = _np(got["silence_default"][0]), _np(got["silence_low"][0])
    quiet = [t for t in range(f_def.shape[1]) if t * R.HOP - R.FRAME // 2 >= R.SILENCE_STEP]
    assert len(quiet) >= 10 and not f_def[0, quiet].any() and (f_low[0, quiet] > 0).all()
    assert (f_def[1] > 0).all() and (f_low[1] > 0).all(), "utterance 1 is above 0.03 x its own peak, below 0.03 x utterance 0's"
    sel = R.full_window_frames(R.GROUND_TRUTH_N)
    assert not _np(got["voicing_default"][0]).any() and (_np(got["voicing_low"][0])[0, sel] > 0).all()


# ------------------------------------------------------------------------------------------------------------------ target chain at its size edges
def _check_norm_interp(name, f0, frames):
    y, uv = K.norm_interp_f0(_dev(f0), _i32(frames))
    y64, uv64 = R.norm_interp_f0_batch(f0, frames)
    y32, _ = R.norm_interp_f0_batch(f0, frames, dtype=np.float32)
    assert np.array_equal(_np(uv), uv64.astype(np.float32))
    e = np.abs(_np(y).astype(np.float64) - y64).max()
    twin = np.abs(y32.astype(np.float64) - y64).max()
    print(f"{name} norm_interp_f0: abs err {e:.3e} (twin {twin:.3e})")
    assert np.isfinite(_np(y)).all() and e <= TWIN_X * twin
    for b, n in enumerate(frames):
        assert not _np(y)[b, n:].any() and not _np(uv)[b, n:].any(), "frames beyond the length must be exactly 0"
    return y, uv


def _check_batch_independence(f0, frames, t, y, uv):
    """each utterance against its own B = 1 call at its own length: M = 2^ceil(log2 n) and CH = ceil(n / 256) are per utterance"""
    d = _dev(f0)
    for b, n in enumerate(frames):
        row = d[b:b + 1, :n].contiguous()
        t1 = PF.f0_targets(row, _i32([n]))
        for key in ("uv", "cont_lf0", "cwt_spec"):
            assert torch.equal(t1[key][0], t[key][b, :n]), (b, key)
        for key in ("f0_mean", "f0_std", "valid"):
            assert torch.equal(t1[key][0], t[key][b]), (b, key)
        y1, uv1 = K.norm_interp_f0(row, _i32([n]))
        assert torch.equal(y1[0], y[b, :n]) and torch.equal(uv1[0], uv[b, :n]), b


def test_chain_size_edges():
    """n = 2, 3 (M = 2, 4), 255 / 256 / 257 (the step from CH = 1 to 2, and from M = 256 to 512), 512 / 513, 2048 / 2049"""
    for f0, frames in R.gpu_chain_edge_batches():
        name = f"edges F={f0.shape[1]}"
        t = _check_chain(name, f0, frames)
        assert _np(t["valid"]).tolist() == [int(n != 2) for n in frames]  # two frames: pycwt's normalisation is NaN at M = 2
        y, uv = _check_norm_interp(name, f0, frames)
        _check_batch_independence(f0, frames, t, y, uv)


def test_chain_long_unvoiced_runs():
    """n = 4096 (16 frames per chunk): the nearest voiced neighbour is carried across up to 255 chunk summaries"""
    f0, frames = R.gpu_chain_long_runs()
    t = _check_chain("long runs", f0, frames)
    assert _np(t["valid"]).tolist() == [1, 1, 1, 1, 0]                    # the last: one voiced frame, a constant contour
    y, uv = _check_norm_interp("long runs", f0, frames)
    _check_batch_independence(f0, frames, t, y, uv)


# ------------------------------------------------------------------------------------------------------------------ composition, capture
TARGET_KEYS = ("pitch", "f0", "uv", "cwt_spec", "f0_mean", "f0_std", "valid")


def _restated_targets(c, dtype):
    """the chain pitch_targets_from_wav composes: tracker -> frames = 1 + lens // hop -> f0_targets, norm_interp_f0"""
    hop = c["params"].get("hop", R.HOP)
    f0, _ = R.track_pitch(c["wav"], c["lens"], dtype=dtype, **c["params"])
    frames = [1 + int(n) // hop for n in c["lens"]]
    t = R.f0_targets(f0, frames, dtype=dtype)
    y, _ = R.norm_interp_f0_batch(f0, frames, dtype=dtype)
    return dict(t, pitch=f0, f0=y), frames


@pytest.mark.parametrize("name", ["ragged", "ragged_sr16k"])
def test_pitch_targets_from_wav_against_float64(cases, name):
    c = cases[name]
    p = dict(c["params"])
    sr, hop = p.pop("sr", R.SR), p.pop("hop", R.HOP)
    stft = ctts_amd.TacotronSTFT(1024, hop, 1024 if hop == 256 else 800, 80, sr, 0, 8000)
    assert (stft.sampling_rate, stft.hop) == (sr, hop)
    got = PF.pitch_targets_from_wav(_dev(c["wav"]), _i32(c["lens"]), stft, **p)
    r64, frames = _restated_targets(c, np.float64)
    r32, _ = _restated_targets(c, np.float32)
    assert got["pitch"].shape == (5, 1 + c["wav"].shape[1] // hop) and got["mel2ph"] is None
    assert r64["valid"].tolist() == [1, 0, 1, 0, 1] and np.array_equal(r32["valid"], r64["valid"])
    assert np.array_equal(_np(got["valid"]), r64["valid"]) and got["valid"].dtype == torch.int32
    assert np.array_equal(_np(got["uv"]), r64["uv"].astype(np.float32)) and np.array_equal(r32["uv"], r64["uv"])
    v = r64["pitch"] > 0
    assert np.array_equal(_np(got["pitch"]) > 0, v) and np.array_equal(r32["pitch"] > 0, v)
    e = (np.abs(_np(got["pitch"]).astype(np.float64) - r64["pitch"])[v] / r64["pitch"][v]).max()
    twin = (np.abs(r32["pitch"].astype(np.float64) - r64["pitch"])[v] / r64["pitch"][v]).max()
    print(f"targets {name} pitch: rel err {e:.3e} (twin {twin:.3e})")
    assert e <= max(TWIN_X * twin, F0_REL_FLOOR)
    for key in ("f0", "cwt_spec", "f0_mean", "f0_std"):
        g = _np(got[key])
        assert g.dtype == np.float32 and g.shape == r64[key].shape and np.isfinite(g).all(), key
        e = np.abs(g.astype(np.float64) - r64[key]).max()
        twin = np.abs(r32[key].astype(np.float64) - r64[key]).max()
        print(f"targets {name} {key}: abs err {e:.3e} (twin {twin:.3e}), max |ref| {np.abs(r64[key]).max():.3g}")
        assert e <= TWIN_X * twin, key
    for b, n in enumerate(frames):
        for key in ("pitch", "f0", "uv", "cwt_spec"):
            assert not _np(got[key])[b, max(n, 0):].any(), "frames beyond 1 + len // hop must be exactly 0"


def test_pitch_targets_are_capturable(cases):
    """one captured pitch_targets_from_wav on static buffers, replayed on a second batch with other lengths: bit-identical to the eager
    call on that batch; the workspace cannot be built inside a capture"""
    stft = ctts_amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    first = (cases["ragged"]["wav"], (6000, 100, 6144, 0, 3333))
    second = (np.ascontiguousarray(cases["ground_truth"]["wav"][:5]), (6144, 5000, 2999, 6100, 700))
    PF.prepare(DEV)
    wav, lens = _dev(first[0]).clone(), _i32(first[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        PF.pitch_targets_from_wav(wav, lens, stft)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = PF.pitch_targets_from_wav(wav, lens, stft)
    for w, n in (first, second, first):
        wav.copy_(_dev(w))
        lens.copy_(_i32(n))
        for key in TARGET_KEYS:
            captured[key].fill_(7)
        g.replay()
        torch.cuda.synchronize()
        eager = PF.pitch_targets_from_wav(_dev(w), _i32(n), stft)
        for key in TARGET_KEYS:
            assert torch.equal(captured[key], eager[key]), key
        assert (eager["pitch"] > 0).any() and eager["valid"].any()
    saved = dict(PF._WS)
    PF._WS.clear()
    try:
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2):
            lens.add_(0)                                                   # the capture is a real one and holds a node
            with pytest.raises(_lib.CttsError, match="before capturing a graph"):
                PF.prepare(DEV)
        assert not PF._WS
    finally:
        PF._WS.update(saved)
    torch.cuda.synchronize()
    f0, _ = PF.track_pitch(_dev(first[0]), _i32(first[1]))                # the workspace is back and usable
    assert torch.equal(f0, PF.pitch_targets_from_wav(_dev(first[0]), _i32(first[1]), stft)["pitch"])
