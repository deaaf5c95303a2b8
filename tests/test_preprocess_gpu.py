"""GPU: the dataset-preparation kernels (csrc/preprocess.hip through ctts_amd.preprocess) against the float64 restatements of
tests/preprocess_restate.py and the live reference's results (tests/golden/g20_preprocess.npz), the batch driver `process_batch`
against the kernels it chains, and the `attn_prior="device"` data path against host-computed priors.

Bars.  Trim: start / end exactly equal - the test first asserts that no frame of its own signals lies within 0.01 dB of the threshold
in the float64 restatement; frame powers within 1e-6 relative of float64.  Prior: relative <= 1e-6 where the reference is >= 1e-30,
absolute <= 1e-37 below (tests/test_preprocess_restate_cpu.py derives it), log(prior + 1e-8) absolute <= 1e-6, padding exactly 0.
Outlier filter: keep / count / min / max exact - the test asserts that none of its values lies within 1e-5 (relative) of a bound;
sum, M2 and the merged mean / std relative <= 1e-9 (double accumulation on the device).

One definition differs from a parenthesis of the feature request: an all-zero utterance has mse_f = ref = 0, so every frame is 0 dB
below the reference and NOTHING is trimmed - (0, len), not (0, 0) - by the stated formula and in librosa alike.  The case is kept and
checked against the restatement like every other."""
import numpy as np
import pytest
import torch

import ctts_amd
from ctts_amd import audio, data as D, preprocess as PP
from ctts_amd._lib import CttsError
from ctts_amd.configs import get_configs
from tests import preprocess_restate as R
from tests.preprocess_restate import assert_prior_close
from tests.util import load_golden, synthetic_samples

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HOP, FRAME = 256, 1024


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------- silence trim
TRIM_LENS = [513, 1024, 4000, 22050, 22051]
TRIM_KINDS = ["zero", "loud", "edges", "burst"]


def trim_signal(kind, n, seed):
    rng = np.random.default_rng(seed)
    tone = 0.5 * np.sin(np.arange(n) * 0.37 + 0.1)
    if kind == "zero":
        return np.zeros(n, dtype=np.float32)
    if kind == "loud":
        return tone.astype(np.float32)
    x = 1e-4 * rng.standard_normal(n)                       # -71 dB below the tone's power: silent at top_db 23 and 60
    if kind == "edges":                                     # leading and trailing silence, neither edge on a multiple of hop
        a, b = int(0.31 * n) | 1, int(0.68 * n) | 1
        x[a:b] = tone[a:b]
    else:                                                   # a burst only inside the last partial frame (the last 64 samples when len % hop == 0)
        a = n - max(n % HOP, 64) + 7
        x[a:n - 3] = tone[a:n - 3]
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def trim_batch():
    rows = [(k, n) for n in TRIM_LENS for k in TRIM_KINDS]
    sigs = [trim_signal(k, n, 40 + i) for i, (k, n) in enumerate(rows)]
    N = max(TRIM_LENS) + 77
    rng = np.random.default_rng(7)
    host = rng.uniform(-1.0, 1.0, (len(rows), N)).astype(np.float32)          # loud noise at and beyond lens[b]: must never be read
    for i, s in enumerate(sigs):
        host[i, :len(s)] = s
    db = [R.frame_db(s.astype(np.float64), FRAME, HOP) for s in sigs]
    mse = [R.frame_power(s.astype(np.float64), FRAME, HOP) for s in sigs]
    return rows, sigs, host, db, mse


@pytest.mark.parametrize("top_db", [23, 60])
def test_trim_silence_matches_restatement_exactly(trim_batch, top_db):
    rows, sigs, host, db, mse64 = trim_batch
    for (k, n), d in zip(rows, db):                         # the condition under which exact equality is a fair demand
        assert np.abs(d + top_db).min() > 0.01, (k, n, np.abs(d + top_db).min())
    want = [R.trim_silence(s.astype(np.float64), top_db, FRAME, HOP) for s in sigs]
    lens = [len(s) for s in sigs]
    wav = torch.from_numpy(host).to(DEV)
    start, end, dur, mse = PP.trim_silence(wav, dev_i32(lens), top_db, FRAME, HOP, return_power=True)
    got = list(zip(start.tolist(), end.tolist()))
    print("trim", top_db, {f"{k}{n}": g for (k, n), g in zip(rows, got)})
    assert got == want
    assert dur.tolist() == [(e - s) // HOP for s, e in want]
    for (k, n), w in zip(rows, want):
        if k == "zero" or k == "loud":
            assert w == (0, n), (k, n, w)
        if k == "edges" and n >= 4000:
            assert 0 < w[0] and w[1] < n and w[0] % HOP == 0
    mse = mse.cpu().numpy().astype(np.float64)
    worst = 0.0
    for i, m in enumerate(mse64):
        nz = m > 0
        assert np.all(mse[i, :len(m)][~nz] == 0)
        worst = max(worst, float((np.abs(mse[i, :len(m)][nz] - m[nz]) / m[nz]).max()) if nz.any() else 0.0)
        assert np.all(mse[i, len(m):] == 0)
    print(f"trim: frame power max relative error vs float64 {worst:.3e}")
    assert worst <= 1e-6
    # the region at and beyond lens[b] does not matter, and host-given lengths take the same path
    host2 = host.copy()
    for i, n in enumerate(lens):
        host2[i, n:] = 0.99
    s2, e2, d2 = PP.trim_silence(torch.from_numpy(host2).to(DEV), lens, top_db, FRAME, HOP)
    assert torch.equal(s2, start) and torch.equal(e2, end) and torch.equal(d2, dur)


def test_trim_silence_argument_checks():
    wav = torch.zeros(2, 2000, device=DEV)
    with pytest.raises(ValueError):
        PP.trim_silence(wav, [512, 2000], 23)               # reflection needs more than frame_length / 2 samples
    with pytest.raises(ValueError):
        PP.trim_silence(wav, [2001, 2000], 23)
    with pytest.raises(CttsError):
        PP.trim_silence(wav.cpu(), [2000, 2000], 23)
    s, e, d = PP.trim_silence(wav, dev_i32([0, 5000]), 23)  # device-given lengths are clamped: 0 -> (0, 0), 5000 -> N
    assert s.tolist() == [0, 0] and e.tolist() == [0, 2000]


# ---------------------------------------------------------------------------------------------------------------------- alignment prior
PRIOR_SRC, PRIOR_MEL, PRIOR_TS, PRIOR_TM = [1, 3, 7, 55, 128], [1, 7, 3, 440, 1000], 128, 1024


@pytest.fixture(scope="module")
def prior_ref():
    return {sf: R.attention_prior_batch(PRIOR_SRC, PRIOR_MEL, PRIOR_TS, PRIOR_TM, sf) for sf in (1.0, 0.5)}


@pytest.mark.parametrize("sf", [1.0, 0.5])
def test_attention_prior_matches_restatement_and_reference(prior_ref, sf):
    ref = prior_ref[sf]
    B = len(PRIOR_SRC)
    out = torch.full((B, PRIOR_TS, PRIOR_TM), float("nan"), device=DEV)
    ret = PP.attention_prior(dev_i32(PRIOR_SRC), dev_i32(PRIOR_MEL), sf, out=out)
    assert ret.data_ptr() == out.data_ptr()
    got = out.cpu().numpy()
    assert np.isfinite(got).all()                           # every element written
    valid = (np.arange(PRIOR_TS)[None, :, None] < np.array(PRIOR_SRC)[:, None, None]) & \
            (np.arange(PRIOR_TM)[None, None, :] < np.array(PRIOR_MEL)[:, None, None])
    assert np.all(got[~valid] == 0)                         # the padding is exactly zero
    for b in range(B):
        p, m = PRIOR_SRC[b], PRIOR_MEL[b]
        assert_prior_close(got[b, :p, :m], ref[b, :p, :m].astype(np.float32), f"kernel vs restatement ({p},{m}) sf {sf}")
    err = np.abs(np.log(got.astype(np.float64)[valid] + 1e-8) - np.log(ref[valid] + 1e-8)).max()
    print(f"prior sf {sf}: log(prior + 1e-8) max abs error {err:.3e}")
    assert err <= 1e-6
    if sf == 1.0:                                           # the live reference's own numbers
        g = load_golden("g20_preprocess")
        for b, key in ((0, "prior_1_1_1.0"), (1, "prior_7_3_1.0"), (2, "prior_3_7_1.0"), (3, "prior_440_55_1.0")):
            assert_prior_close(got[b, :PRIOR_SRC[b], :PRIOR_MEL[b]], g[key], f"kernel vs reference {key}")
        assert_prior_close(got[4, list(g["prior_big_rows"]), :1000], g["prior_big"], "kernel vs reference 1000x128 rows")
    # allocating call: same numbers, host lengths
    again = PP.attention_prior(PRIOR_SRC, PRIOR_MEL, sf, max_src_len=PRIOR_TS, max_mel_len=PRIOR_TM)
    assert torch.equal(again, out)


def test_attention_prior_writes_into_a_view_and_nowhere_else():
    src, mel, Ts, Tm = [3, 7, 5], [7, 3, 20], 7, 20
    big = torch.full((5, Ts + 1, Tm + 3), float("nan"), device=DEV)
    view = big[1:4, :Ts, 2:Tm + 2]
    PP.attention_prior(dev_i32(src), dev_i32(mel), 1.0, out=view)
    h = big.cpu().numpy()
    inside = np.zeros(h.shape, dtype=bool)
    inside[1:4, :Ts, 2:Tm + 2] = True
    assert np.isnan(h[~inside]).all() and np.isfinite(h[inside]).all()
    ref = R.attention_prior_batch(src, mel, Ts, Tm)
    for b in range(3):
        assert_prior_close(h[1 + b, :src[b], 2:2 + mel[b]], ref[b, :src[b], :mel[b]].astype(np.float32), f"view row {b}")
    with pytest.raises(CttsError):
        PP.attention_prior(dev_i32(src), dev_i32(mel), 1.0)                    # device lengths: the padded shape must be given
    with pytest.raises(CttsError):
        PP.attention_prior(dev_i32(src), dev_i32(mel), 1.0, out=torch.empty(3, Ts, Tm))
    with pytest.raises(CttsError):
        PP.attention_prior(dev_i32(src), dev_i32(mel), 0.0, out=big[1:4, :Ts, 2:Tm + 2])


# ---------------------------------------------------------------------------------------------------------------------- outlier filter
@pytest.fixture(scope="module")
def outlier_rows():
    rng = np.random.default_rng(77)
    rows = dict(R.outlier_fixtures())                       # 1, 2, 3, 4, 5, 101, 870, constant, ties - also stored with the reference's answers
    for n in (64, 65, 4096):
        v = rng.normal(37.0, 9.0, n)
        idx = rng.choice(n, n // 32, replace=False)
        v[idx] += rng.choice([-1.0, 1.0], len(idx)) * rng.uniform(60.0, 200.0, len(idx))
        rows[f"n{n}"] = v.astype(np.float32)
    rows["ties4096"] = np.round(rng.normal(-0.5, 4.0, 4096)).astype(np.float32)        # integers: long runs of equal values at both quartiles
    return rows


def test_outlier_stats_match_restatement_and_reference(outlier_rows):
    names, L = list(outlier_rows), 4096
    assert sorted({len(v) for v in outlier_rows.values()} & {1, 2, 3, 4, 5, 64, 65, 870, 4096}) == [1, 2, 3, 4, 5, 64, 65, 870, 4096]
    host = np.full((len(names), L), 1e30, dtype=np.float32)                 # garbage at and beyond lens[b]
    for i, k in enumerate(names):
        assert R.bound_margin(outlier_rows[k]) > 1e-5, (k, R.bound_margin(outlier_rows[k]))
        host[i, :len(outlier_rows[k])] = outlier_rows[k]
    lens = [len(outlier_rows[k]) for k in names]
    o = PP.outlier_stats(torch.from_numpy(host).to(DEV), dev_i32(lens))
    keep, count = o["keep"].cpu().numpy(), o["count"].cpu().numpy()
    s, m2, lo, hi = (o[k].cpu().numpy() for k in ("sum", "M2", "min", "max"))
    assert keep.dtype == np.uint8 and s.dtype == np.float64 and m2.dtype == np.float64
    g = load_golden("g20_preprocess")
    for i, k in enumerate(names):
        v, n = outlier_rows[k], lens[i]
        want = R.outlier_keep(v)
        assert np.array_equal(keep[i, :n].astype(bool), want), k
        assert not keep[i, n:].any(), k
        assert count[i] == want.sum(), k
        if f"out_{k}_kept" in g:
            assert np.array_equal(v[keep[i, :n].astype(bool)], g[f"out_{k}_kept"]), k
        c, ws, wm2 = R.moments(v)
        if c == 0:
            assert s[i] == 0 and m2[i] == 0 and lo[i] == np.inf and hi[i] == -np.inf, k
            continue
        assert abs(s[i] - ws) <= 1e-9 * abs(ws), (k, s[i], ws)
        assert abs(m2[i] - wm2) <= 1e-9 * abs(wm2), (k, m2[i], wm2)
        assert lo[i] == v[want].min() and hi[i] == v[want].max(), k
    assert count[names.index("const")] == 0 and count[names.index("n1")] == 0
    n, mean, std = PP.merge_moments(count, s, m2)
    wmean, wstd = R.dataset_mean_std([outlier_rows[k] for k in names])
    print(f"outlier stats: {n} kept of {sum(lens)}; mean {mean!r} vs {wmean!r}; std {std!r} vs {wstd!r}")
    assert abs(mean - wmean) <= 1e-9 * abs(wmean) and abs(std - wstd) <= 1e-9 * abs(wstd)
    # the reference's scaler, fed the stored fixtures in their order
    fx = list(g["out_order"])
    idx = [names.index(k) for k in fx]
    _, mean, std = PP.merge_moments(count[idx], s[idx], m2[idx])
    assert abs(mean - g["scaler_mean"][0]) <= 1e-9 * abs(g["scaler_mean"][0])
    assert abs(std - g["scaler_scale"][0]) <= 1e-9 * abs(g["scaler_scale"][0])


def test_outlier_stats_refuses_more_than_4096_values():
    with pytest.raises(CttsError, match="4096"):
        PP.outlier_stats(torch.zeros(1, 4097, device=DEV), dev_i32([4097]))
    with pytest.raises(CttsError):
        PP.outlier_stats(torch.zeros(1, 8), [8])


def test_dataset_stats_follow_the_reference_rules(outlier_rows):
    """energy: mean / std over the kept values, min / max over ALL stored values after normalisation; f0: over the non-zero frames"""
    names = ["n101", "n870", "n65"]
    L = 870
    e = np.zeros((3, L), dtype=np.float32)
    for i, k in enumerate(names):
        e[i, :len(outlier_rows[k])] = outlier_rows[k]
    lens = [len(outlier_rows[k]) for k in names]
    rng = np.random.default_rng(5)
    f0 = (rng.uniform(80, 400, (3, L)) * (rng.random((3, L)) > 0.4)).astype(np.float32)
    mel = rng.normal(-5, 2, (3, L, 80)).astype(np.float32)
    st = PP.DatasetStats("unsup")
    st.update(dev_i32(lens[:2]), energy=torch.from_numpy(e[:2]).to(DEV), f0=torch.from_numpy(f0[:2]).to(DEV), mel=torch.from_numpy(mel[:2]).to(DEV))
    st.update(dev_i32(lens[2:]), energy=torch.from_numpy(e[2:]).to(DEV), f0=torch.from_numpy(f0[2:]).to(DEV), mel=torch.from_numpy(mel[2:]).to(DEV))
    out = st.finalize()
    assert set(out) == {"f0_unsup", "energy_unsup_frame", "spec_unsup_min", "spec_unsup_max", "max_seq_len"}
    wmean, wstd = R.dataset_mean_std([outlier_rows[k] for k in names])
    allv = np.concatenate([outlier_rows[k].astype(np.float64) for k in names])
    want = [(allv.min() - wmean) / wstd, (allv.max() - wmean) / wstd, wmean, wstd]
    assert np.allclose(out["energy_unsup_frame"], want, rtol=1e-9, atol=0)
    v = np.concatenate([f0[i, :n] for i, n in enumerate(lens)]).astype(np.float64)
    v = v[v != 0]
    assert np.allclose(out["f0_unsup"], [v.mean(), v.std()], rtol=1e-9, atol=0)
    mm = np.concatenate([mel[i, :n] for i, n in enumerate(lens)])
    assert out["spec_unsup_min"] == mm.min(0).astype(np.float64).tolist() and out["spec_unsup_max"] == mm.max(0).astype(np.float64).tolist()
    assert out["max_seq_len"] == 870


# ---------------------------------------------------------------------------------------------------------------------- process_batch
def speechlike(n, seed, lead, trail):
    """a gliding fundamental with harmonics under a syllable envelope between `lead` and `n - trail`, faint noise outside"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    f = 140.0 + 40.0 * np.sin(2 * np.pi * 0.9 * t + seed) + 20.0 * np.sin(2 * np.pi * 2.3 * t)
    ph = 2 * np.pi * np.cumsum(f) / 22050.0
    x = 0.3 * sum(np.sin(k * ph) / k for k in range(1, 6)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t + seed))
    y = 1e-4 * rng.standard_normal(n)
    y[lead:n - trail] = x[lead:n - trail]
    return np.clip(y, -1, 1).astype(np.float32)


def test_process_batch_equals_the_kernels_it_chains():
    stft = audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(DEV)
    pre, _, _ = get_configs()
    pre["preprocessing"]["audio"]["trim_top_db"] = 23
    pre["preprocessing"]["duration"] = {"beta_binomial_scaling_factor": 1.0}
    wavs = [speechlike(22050, 1, 3001, 2501), speechlike(20011, 2, 1777, 4099), speechlike(24577, 3, 5003, 1201)]
    nph = [11, 7, 15]
    for w in wavs:
        assert np.abs(R.frame_db(w.astype(np.float64)) + 23).min() > 0.01
    spans = [R.trim_silence(w.astype(np.float64), 23) for w in wavs]
    dwavs = [torch.from_numpy(w).to(DEV) for w in wavs]
    out = PP.process_batch(dwavs, nph, stft, pre)
    slices = [w[s:e] for w, (s, e) in zip(wavs, spans)]
    mels = stft.mel_spectrograms_ragged(slices)
    n = max(len(s) for s in slices)
    pad = np.zeros((3, n), dtype=np.float32)
    for i, s in enumerate(slices):
        pad[i, :len(s)] = s
    tl = dev_i32([len(s) for s in slices])
    pt = ctts_amd.pitch_targets_from_wav(torch.from_numpy(pad).to(DEV), tl, stft)
    durs = [(e - s) // HOP for s, e in spans]
    prior = PP.attention_prior(nph, durs, 1.0).cpu().numpy()
    from ctts_amd.model import f0_to_coarse
    coarse = f0_to_coarse(pt["pitch"]).cpu().numpy()
    pt = {k: v.cpu().numpy() for k, v in pt.items() if torch.is_tensor(v)}
    for b, o in enumerate(out):
        T = durs[b]
        assert (o["start"], o["end"]) == spans[b] and o["duration"] == T and 50 < T < 100
        assert o["mel"].shape == (T, 80) and o["mel"].shape[0] == o["energy"].shape[0] == o["f0"].shape[0] == o["attn_prior"].shape[1]
        assert np.array_equal(o["mel"], mels[b][0][:, :T].T) and np.array_equal(o["energy"], mels[b][1][:T])
        assert np.array_equal(o["f0"], pt["pitch"][b, :T]) and (o["f0"] > 0).sum() > 20
        assert np.array_equal(o["pitch"], coarse[b, :T])
        assert np.array_equal(o["cwt_spec"], pt["cwt_spec"][b, :T]) and o["cwt_spec"].shape == (T, 10)
        assert np.array_equal(o["f0cwt_mean_std"], np.array([pt["f0_mean"][b], pt["f0_std"][b]]))
        assert o["valid"] == int(pt["valid"][b]) == 1
        assert o["attn_prior"].shape == (nph[b], T) and np.array_equal(o["attn_prior"], prior[b, :nph[b], :T])
    again = PP.process_batch(dwavs, nph, stft, pre)
    given = PP.process_batch(dwavs, nph, stft, pre, spans=spans)           # explicit spans replace the trim
    for o, a, s in zip(out, again, given):
        for k, v in o.items():
            assert np.array_equal(v, a[k]) and np.array_equal(v, s[k]), k
    with pytest.raises(CttsError):
        PP.process_batch([torch.from_numpy(w) for w in wavs], nph, stft, pre)


# ---------------------------------------------------------------------------------------------------------------------- data path
def test_device_prior_data_path_matches_host_priors_and_feeds_c5():
    samples = synthetic_samples(6, 11, True)
    for s in samples:                                       # the files a preprocessing run would have written: the restated prior
        s["attn_prior"] = R.attention_prior(s["text"].shape[0], s["mel"].shape[0]).astype(np.float32)
    stripped = [{k: v for k, v in s.items() if k != "attn_prior"} for s in samples]
    b_files = D.collate(samples, 6, sort=True, learn_alignment=True)[0]
    b_dev = D.collate(stripped, 6, sort=True, learn_alignment=True, attn_prior="device")[0]
    assert b_dev[18] is None
    files, ev = D.PackedBatch.pack(b_files).to_device(DEV)
    ev.synchronize()
    pb = D.PackedBatch.pack(b_dev, attn_prior="device")
    dev, ev = pb.to_device(DEV)
    ev.synchronize()
    assert pb.device_buffer.numel() == pb.device_bytes and dev[12].data_ptr() == pb.device_buffer.data_ptr() + pb.device_layout["attn_priors"][0]
    want, got = files[12].cpu().numpy(), dev[12].cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    src, mel = files[4].tolist(), files[7].tolist()
    for b in range(len(src)):
        assert_prior_close(got[b, :src[b], :mel[b]], want[b, :src[b], :mel[b]], f"device prior of utterance {b}")
    assert np.all(got[want == 0] == 0)
    for a, b_ in zip(files, dev):                           # every other field is the same upload
        if torch.is_tensor(a) and a is not files[12]:
            assert torch.equal(a, b_)
    via_prefetcher = list(D.Prefetcher([b_dev], DEV, attn_prior="device"))[0]
    torch.cuda.current_stream().synchronize()
    assert torch.equal(via_prefetcher[12], dev[12])
    # config C5 (liu2021 prosody + learn_alignment) forward on both
    torch.manual_seed(4)
    pre, mc, tc = get_configs()
    mc["prosody_modeling"]["model_type"] = "liu2021"
    mc["duration_modeling"]["learn_alignment"] = True
    m = ctts_amd.CompTransTTS(pre, mc, tc).to(DEV)
    m.train()
    for sub in m.modules():
        if hasattr(sub, "dropout"):
            sub.dropout = 0.0
    with torch.no_grad():
        o1 = m(*files[2:], step=100001)
        o2 = m(*dev[2:], step=100001)
    err = float((o1[1] - o2[1]).abs().max())
    print(f"C5 postnet_mel, host priors vs device priors: max abs {err:.3e}")
    assert torch.isfinite(o2[1]).all() and err <= 1e-5


def test_synthetic_unsup_batch_with_the_real_prior():
    from ctts_amd.synthetic import make_unsup_batch, to_device
    band, real = make_unsup_batch([9, 5], 4), make_unsup_batch([9, 5], 4, prior="beta_binomial", scaling_factor=0.5)
    assert real["attn_priors"] is None and band["attn_priors"] is not None
    assert torch.equal(band["e_targets"], real["e_targets"]) and torch.equal(band["mels"], real["mels"])
    d = to_device(real, DEV)
    ref = R.attention_prior_batch([9, 5], real["mel_lens"].tolist(), 9, int(real["mel_lens"].max()), 0.5)
    got = d["attn_priors"].cpu().numpy()
    assert got.shape == ref.shape
    for b, (p, m_) in enumerate(zip([9, 5], real["mel_lens"].tolist())):
        assert_prior_close(got[b, :p, :m_], ref[b, :p, :m_].astype(np.float32), f"synthetic prior {b}")
    assert np.all(got[ref == 0] == 0)
