"""GPU: the objective-evaluation kernels (csrc/metrics.hip through ctts_amd.metrics) against the float64 restatement of
tests/metrics_restate.py.

Bars (derived, not fitted).
  Cepstrum: absolute <= (M + 4) 2^-24 sum_m |mel[m]| sqrt(2/M) per coefficient - the rounding of an M-term fp32 dot product (one rounding
  per table entry, one per fused multiply-add) with |cos| <= 1.  Padding rows exactly 0.
  DTW cost: relative <= (Lx + Ly + K + 4) 2^-23 against the float64 optimum.  Every path sums fewer than Lx + Ly fp32 local costs, each
  carrying about K + 2 roundings of 2^-24, so the fp32 and the float64 minimum differ by at most the worst path's rounding,
  (Lx + Ly + K + 2) 2^-24 relative; the bar is twice that.
  DTW path: the fp32 kernel and the float64 restatement may choose different paths on a near-tie, so paths are not compared cell by
  cell: the kernel's path must be a monotone path from (0,0) to (Lx-1, Ly-1) whose float64 cost is <= optimum x (1 + the cost bar).
  Where the optimum is unique by construction (identical sequences, every frame repeated twice) the path is compared exactly.
  Path sums: counts exact, the squared sum relative <= 1e-9 (double accumulation on the device, float64 log2 on both sides).
Rows at and beyond every length hold NaN in every input: a kernel that reads one of them as data fails these tests."""
import numpy as np
import pytest
import torch

from ctts_amd import audio, metrics as M
from ctts_amd._lib import CttsError
from tests import metrics_restate as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

RAGGED = [(1, 1), (1, 7), (7, 1), (2, 2), (63, 65), (64, 64), (65, 63), (1, 300), (257, 255), (300, 120), (0, 5), (5, 0)]
IDENT = [65, 129]            # identical sequences: pairs 12, 13; every frame repeated twice: pairs 14, 15
T_PAD, K_SMALL = 320, 13
BIG = (1024, 1000, 32)       # one pair at 8 rows per thread, padded to 1030 x 1003
SUBSET = [1, 4, 6, 10, 11, 13]      # re-run at 1 and at 4 rows per thread


def same(a, b):
    """bit-equal, NaN in the same places"""
    return a.dtype == b.dtype and torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def cost_bar(Lx, Ly, K):
    return (Lx + Ly + K + 4) * 2.0 ** -23


def sequences(rng, Lx, Ly, K):
    """a random walk and a time-warped, noisy copy of it: neighbouring frames are close, as cepstra of speech are"""
    x = np.cumsum(rng.standard_normal((Lx, K)), axis=0) * 0.3 + rng.standard_normal((Lx, K))
    if Lx == 0 or Ly == 0:
        return x.astype(np.float32), rng.standard_normal((Ly, K)).astype(np.float32)
    pos = np.clip(np.round(np.linspace(0, Lx - 1, Ly) + rng.uniform(-2, 2, Ly)), 0, Lx - 1).astype(int)
    y = x[np.sort(pos)] + 0.5 * rng.standard_normal((Ly, K))
    return x.astype(np.float32), y.astype(np.float32)


def pad_nan(seqs, T):
    out = np.full((len(seqs), T, seqs[0].shape[1]), np.nan, dtype=np.float32)
    for b, s in enumerate(seqs):
        out[b, :len(s)] = s
    return out


@pytest.fixture(scope="module")
def ragged():
    """the pairs, their float64 optimum and local costs (computed once), and the kernel's answer at the 320 x 320 padding"""
    rng = np.random.default_rng(2024)
    xs, ys = [], []
    for Lx, Ly in RAGGED:
        x, y = sequences(rng, Lx, Ly, K_SMALL)
        xs.append(x), ys.append(y)
    for L in IDENT:
        x = rng.standard_normal((L, K_SMALL)).astype(np.float32)
        xs.append(x), ys.append(x.copy())
    for L in IDENT:
        x = rng.standard_normal((L, K_SMALL)).astype(np.float32)
        xs.append(x), ys.append(np.repeat(x, 2, axis=0))
    ref = []
    for x, y in zip(xs, ys):
        if len(x) == 0 or len(y) == 0:
            ref.append((None, 0.0))
            continue
        d = R.local_cost(x, y)
        ref.append((d, float(R.accumulate_fast(d)[-1, -1])))
    lx, ly = [len(x) for x in xs], [len(y) for y in ys]
    got = run_dtw(xs, ys, T_PAD, T_PAD)
    return {"xs": xs, "ys": ys, "ref": ref, "lx": lx, "ly": ly, "got": got}


def run_dtw(xs, ys, Tx, Ty, align="dtw"):
    x, y = torch.from_numpy(pad_nan(xs, Tx)).to(DEV), torch.from_numpy(pad_nan(ys, Ty)).to(DEV)
    out = M.dtw(x, dev_i32(len(s) for s in xs), y, dev_i32(len(s) for s in ys), align)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_pair(tag, got, b, Lx, Ly, K, d, opt):
    """cost and path of pair b against the float64 local costs d and optimum opt"""
    P = got["path"].shape[1]
    cost, n, path = float(got["cost"][b]), int(got["path_len"][b]), got["path"][b]
    assert np.isfinite(cost)
    if Lx == 0 or Ly == 0:
        assert cost == 0.0 and n == 0 and (path == -1).all(), tag
        return 0.0
    bar = cost_bar(Lx, Ly, K)
    rel = abs(cost - opt) / opt if opt > 0 else abs(cost)
    print(f"{tag} {Lx}x{Ly}: cost {cost:.6f} optimum {opt:.6f} rel {rel:.2e} = {rel / bar:.3f} of the bar {bar:.2e}; path_len {n}")
    assert rel <= bar, (tag, rel, bar)
    assert max(Lx, Ly) <= n <= Lx + Ly - 1 and n <= P, (tag, n)
    assert (path[n:] == -1).all(), tag
    assert (path[:n] >= 0).all(), tag
    assert n == int((path[:, 0] >= 0).sum()), tag
    pl = [tuple(int(v) for v in p) for p in path[:n]]
    assert R.is_monotone_path(pl, Lx, Ly), tag
    assert R.path_cost(d, pl) <= opt * (1.0 + bar), (tag, R.path_cost(d, pl), opt)
    return rel / bar


# ------------------------------------------------------------------------------------------------------------------------ cepstrum
@pytest.mark.parametrize("M_,F,K", [(80, 300, 13), (80, 70, 32), (20, 257, 13), (33, 64, 1)])
def test_mel_cepstrum_matches_float64(M_, F, K):
    rng = np.random.default_rng(M_ + F + K)
    frames = [F, F // 2 + 1, 0, 1]
    mel = rng.uniform(-11.5, 2.0, (len(frames), M_, F)).astype(np.float32)
    for b, n in enumerate(frames):
        mel[b, :, n:] = np.nan
    got = M.mel_cepstrum(torch.from_numpy(mel).to(DEV), dev_i32(frames), K).cpu().numpy()
    assert got.shape == (len(frames), F, K)
    worst = 0.0
    for b, n in enumerate(frames):
        assert (got[b, n:] == 0).all()
        if n == 0:
            continue
        want = R.mel_cepstrum(mel[b, :, :n], K)
        bar = (M_ + 4) * 2.0 ** -24 * np.abs(mel[b, :, :n].astype(np.float64)).sum(0) * np.sqrt(2.0 / M_)
        err = np.abs(got[b, :n] - want)
        worst = max(worst, float((err / bar[:, None]).max()))
        assert (err <= bar[:, None]).all(), (b, float((err / bar[:, None]).max()))
    print(f"cepstrum M={M_} F={F} K={K}: worst error {worst:.3f} of the bar")
    assert np.isfinite(got).all()


def test_mel_cepstrum_closed_forms_and_frames_none():
    M_ = 80
    m = np.arange(M_)
    mel = np.stack([np.full(M_, -3.5), np.cos(np.pi * 5 * (m + 0.5) / M_)], 1)[None].astype(np.float32)      # [1, 80, 2]
    got = M.mel_cepstrum(torch.from_numpy(mel).to(DEV), None, 13).cpu().numpy()[0]
    bar = (M_ + 4) * 2.0 ** -24 * np.abs(mel[0]).sum(0) * np.sqrt(2.0 / M_)
    want = np.zeros((2, 13))
    want[1, 4] = np.sqrt(M_ / 2.0)
    assert (np.abs(got - want) <= bar[:, None] + 2.0 ** -24 * np.sqrt(M_ / 2.0)).all()      # + the float32 rounding of the cosine input itself
    with pytest.raises(CttsError):
        M.mel_cepstrum(torch.zeros(1, 13, 4, device=DEV), None, 13)          # K < M
    with pytest.raises(CttsError):
        M.mel_cepstrum(torch.zeros(1, 80, 4, device=DEV), None, 33)


# ------------------------------------------------------------------------------------------------------------------------ DTW
def test_dtw_ragged_batch_cost_and_path(ragged):
    worst = 0.0
    for b, (Lx, Ly) in enumerate(zip(ragged["lx"], ragged["ly"])):
        d, opt = ragged["ref"][b]
        worst = max(worst, check_pair(f"pair {b}", ragged["got"], b, Lx, Ly, K_SMALL, d, opt))
    print(f"ragged batch: worst cost error {worst:.3f} of the bar")
    assert np.isfinite(ragged["got"]["cost"]).all()


def test_dtw_identical_and_repeated_sequences_are_exact(ragged):
    got, base = ragged["got"], len(RAGGED)
    for k, L in enumerate(IDENT):
        b = base + k
        assert got["cost"][b] == 0.0 and got["path_len"][b] == L
        assert np.array_equal(got["path"][b, :L], np.stack([np.arange(L)] * 2, 1))
        b = base + len(IDENT) + k
        assert got["cost"][b] == 0.0 and got["path_len"][b] == 2 * L
        want = np.stack([np.repeat(np.arange(L), 2), np.arange(2 * L)], 1)
        assert np.array_equal(got["path"][b, :2 * L], want)
        assert (got["path"][b, 2 * L:] == -1).all()


def test_dtw_zero_length_pairs(ragged):
    got = ragged["got"]
    for b, (Lx, Ly) in enumerate(RAGGED):
        if Lx == 0 or Ly == 0:
            assert got["cost"][b] == 0.0 and got["path_len"][b] == 0 and (got["path"][b] == -1).all()
    assert np.isfinite(got["cost"]).all()
    # a batch of nothing but empty pairs
    only = run_dtw([ragged["xs"][10], ragged["xs"][11][:0]], [ragged["ys"][10], ragged["ys"][11][:0]], 8, 8)
    assert (only["cost"] == 0).all() and (only["path_len"] == 0).all() and (only["path"] == -1).all()


@pytest.mark.parametrize("Tx,Ty", [(130, 140), (600, 140)])
def test_dtw_does_not_depend_on_the_padding(ragged, Tx, Ty):
    """the same pairs at 1 and at 4 rows per thread (the fixture runs 2): same cost bits, same path"""
    xs, ys = [ragged["xs"][b] for b in SUBSET], [ragged["ys"][b] for b in SUBSET]
    got = run_dtw(xs, ys, Tx, Ty)
    for k, b in enumerate(SUBSET):
        d, opt = ragged["ref"][b]
        check_pair(f"pad {Tx}x{Ty} pair {b}", got, k, len(xs[k]), len(ys[k]), K_SMALL, d, opt)
        n = int(got["path_len"][k])
        assert got["cost"][k] == ragged["got"]["cost"][b] and n == ragged["got"]["path_len"][b]
        assert np.array_equal(got["path"][k, :n], ragged["got"]["path"][b, :n])


def test_dtw_large_pair_and_determinism():
    Lx, Ly, K = BIG
    rng = np.random.default_rng(77)
    x, y = sequences(rng, Lx, Ly, K)
    d = R.local_cost(x, y)
    opt = float(R.accumulate_fast(d)[-1, -1])
    got = run_dtw([x], [y], 1030, 1003)
    ratio = check_pair("large", got, 0, Lx, Ly, K, d, opt)
    print(f"large pair: cost error {ratio:.3f} of the bar")
    again = run_dtw([x], [y], 1030, 1003)
    for k in ("cost", "path_len", "path"):
        assert np.array_equal(got[k], again[k]), k


def test_dtw_is_deterministic_run_to_run(ragged):
    again = run_dtw(ragged["xs"], ragged["ys"], T_PAD, T_PAD)
    for k in ("cost", "path_len", "path"):
        assert np.array_equal(ragged["got"][k], again[k]), k


def test_dtw_refuses_more_than_2048_padded_frames():
    x, y = torch.zeros(1, 2049, 13, device=DEV), torch.zeros(1, 8, 13, device=DEV)
    n = dev_i32([8])
    with pytest.raises(CttsError):
        M.dtw(x, n, y, n)
    with pytest.raises(CttsError):
        M.dtw(y, n, x, n)
    with pytest.raises(CttsError):
        M.dtw(x, n, y, n, align="none")
    from ctts_amd import _lib, kernels
    c, pl, p = torch.zeros(1, device=DEV), dev_i32([0]), torch.zeros(1, 2056, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(CttsError):                               # the library's own check, in front of every launch
        _lib.check(_lib.load().ctts_dtw(x.data_ptr(), y.data_ptr(), n.data_ptr(), n.data_ptr(), p.data_ptr(), c.data_ptr(), pl.data_ptr(),
                                        p.data_ptr(), 1, 2049, 8, 13, 0, kernels._stream()), "ctts_dtw")
    ok = M.dtw(torch.zeros(1, 2048, 4, device=DEV), dev_i32([3]), torch.zeros(1, 2048, 4, device=DEV), dev_i32([2]))
    assert ok["path_len"].item() == 3 and ok["cost"].item() == 0.0


def test_align_none_is_the_identity_path(ragged):
    got = run_dtw(ragged["xs"], ragged["ys"], T_PAD, T_PAD, align="none")
    for b, (x, y) in enumerate(zip(ragged["xs"], ragged["ys"])):
        n = min(len(x), len(y))
        assert got["path_len"][b] == n
        assert np.array_equal(got["path"][b, :n], np.stack([np.arange(n)] * 2, 1)) and (got["path"][b, n:] == -1).all()
        want = float(np.sqrt(((x[:n].astype(np.float64) - y[:n].astype(np.float64)) ** 2).sum(1)).sum())
        assert abs(float(got["cost"][b]) - want) <= want * (n + K_SMALL + 4) * 2.0 ** -23
    assert np.isfinite(got["cost"]).all()


# ------------------------------------------------------------------------------------------------------------------------ path sums
def f0_tracks(rng, lens, T):
    out = np.full((len(lens), T), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        f = rng.uniform(80.0, 400.0, n)
        f[rng.random(n) < 0.35] = 0.0
        out[b, :n] = f
    return out


def test_path_metrics_on_the_kernels_own_path(ragged):
    rng = np.random.default_rng(5)
    fx, fy = f0_tracks(rng, ragged["lx"], T_PAD), f0_tracks(rng, ragged["ly"], T_PAD)
    path, plen = torch.from_numpy(ragged["got"]["path"]).to(DEV), torch.from_numpy(ragged["got"]["path_len"]).to(DEV)
    out = M.path_metrics(path, plen, torch.from_numpy(fx).to(DEV), torch.from_numpy(fy).to(DEV))
    assert out.dtype == torch.float64 and out.shape == (len(ragged["lx"]), 4)
    again = M.path_metrics(path, plen, torch.from_numpy(fx).to(DEV), torch.from_numpy(fy).to(DEV))
    assert torch.equal(out, again)
    out = out.cpu().numpy()
    assert np.isfinite(out).all()
    seen_voiced = 0
    for b in range(len(ragged["lx"])):
        n = int(ragged["got"]["path_len"][b])
        pairs, both, sq, differ = R.path_metrics([tuple(p) for p in ragged["got"]["path"][b, :n]], fx[b], fy[b])
        assert (out[b, 0], out[b, 1], out[b, 3]) == (pairs, both, differ), b
        assert pairs == n
        assert abs(out[b, 2] - sq) <= 1e-9 * sq, (b, out[b, 2], sq)
        seen_voiced += both
    assert seen_voiced > 200


# ------------------------------------------------------------------------------------------------------------------------ the chain
@pytest.fixture(scope="module")
def mel_pair():
    rng = np.random.default_rng(11)
    B, M_, Fr, Fs = 4, 80, 90, 100
    fr, fs = [90, 41, 0, 77], [100, 37, 12, 77]
    mr, ms = rng.uniform(-11.5, 2.0, (B, M_, Fr)).astype(np.float32), rng.uniform(-11.5, 2.0, (B, M_, Fs)).astype(np.float32)
    ms[3, :, :77] = mr[3, :, :77]
    for b in range(B):
        mr[b, :, fr[b]:] = np.nan
        ms[b, :, fs[b]:] = np.nan
    pr, ps = f0_tracks(rng, fr, Fr), f0_tracks(rng, fs, Fs)
    ps[3, :77] = pr[3, :77]
    t = lambda a: torch.from_numpy(a).to(DEV)       # noqa: E731
    return t(mr), dev_i32(fr), t(ms), dev_i32(fs), t(pr), t(ps)


@pytest.mark.parametrize("align", ["dtw", "none"])
def test_compare_mels_equals_the_chained_calls(mel_pair, align):
    mr, fr, ms, fs, pr, ps = mel_pair
    res = M.compare_mels(mr, fr, ms, fs, pr, ps, align=align)
    a = M.dtw(M.mel_cepstrum(mr, fr), fr, M.mel_cepstrum(ms, fs), fs, align)
    m = M.path_metrics(a["path"], a["path_len"], pr, ps)
    n = a["path_len"].double()
    assert torch.equal(res["path_len"], a["path_len"])
    assert same(res["mcd_db"], M.MCD_DB * a["cost"].double() / n)
    assert same(res["lf0_rmse_cents"], torch.sqrt(m[:, 2] / m[:, 1]))
    assert same(res["vuv_error"], m[:, 3] / n)
    assert torch.equal(res["n_voiced"], m[:, 1].to(torch.int32))
    # the empty reference: NaN measures, counts that say why
    assert res["path_len"][2].item() == 0 and res["n_voiced"][2].item() == 0
    assert all(torch.isnan(res[k][2]) for k in ("mcd_db", "lf0_rmse_cents", "vuv_error"))
    # utterance 3 is compared with itself
    assert res["mcd_db"][3].item() == 0.0 and res["lf0_rmse_cents"][3].item() == 0.0 and res["vuv_error"][3].item() == 0.0
    assert res["path_len"][3].item() == 77
    for k in (0, 1):
        assert res["mcd_db"][k].item() > 0 and np.isfinite(res["mcd_db"][k].item())
    s = M.summarize(res)
    pl, host = res["path_len"].cpu().numpy().astype(np.float64), {k: v.cpu().numpy().astype(np.float64) for k, v in res.items()}
    live = pl > 0
    assert s["mcd_db"].item() == pytest.approx((host["mcd_db"][live] * pl[live]).sum() / pl.sum(), rel=1e-12)
    assert s["vuv_error"].item() == pytest.approx(host["n_mismatch"].sum() / pl.sum(), rel=1e-12)
    assert s["lf0_rmse_cents"].item() == pytest.approx(np.sqrt(host["sq_cents"].sum() / host["n_voiced"].sum()), rel=1e-12)
    assert s["mcd_db"].is_cuda and s["path_len"].item() == pl.sum()


def test_compare_mels_without_f0_and_align_none_on_equal_mels(mel_pair):
    mr, fr, _, _, _, _ = mel_pair
    res = M.compare_mels(mr, fr, mr.clone(), fr, align="none")
    live = fr.cpu().numpy() > 0
    assert (res["mcd_db"].cpu().numpy()[live] == 0.0).all()
    assert torch.equal(res["path_len"], fr)
    assert torch.isnan(res["lf0_rmse_cents"]).all() and torch.isnan(res["vuv_error"]).all() and (res["n_voiced"] == 0).all()
    with pytest.raises(CttsError):
        M.compare_mels(mr, fr, mr, fr, f0_ref=torch.zeros(4, 90, device=DEV))


def test_compare_wavs_of_a_signal_with_itself():
    sr, hop = 22050, 256
    lens = [hop * 40 + 17, hop * 23]
    t = np.arange(max(lens)) / sr
    f = 140.0 + 40.0 * np.sin(2 * np.pi * 1.5 * t)
    ph = 2 * np.pi * np.cumsum(f) / sr
    tone = 0.3 * sum(np.sin(k * ph) / k for k in range(1, 6))
    rng = np.random.default_rng(3)
    wav = np.zeros((2, max(lens)), dtype=np.float32)
    wav[0, :lens[0]] = tone[:lens[0]]
    wav[1, :lens[1]] = np.where(np.arange(lens[1]) < lens[1] // 2, tone[:lens[1]], 0.02 * rng.standard_normal(lens[1]))
    stft = audio.TacotronSTFT(1024, hop, 1024, 80, sr, 0, 8000).to(DEV)
    w, n = torch.from_numpy(wav).to(DEV), dev_i32(lens)
    res = M.compare_wavs(w, n, w.clone(), n, stft)
    assert res["path_len"].tolist() == [1 + v // hop for v in lens]
    assert res["mcd_db"].tolist() == [0.0, 0.0] and res["vuv_error"].tolist() == [0.0, 0.0]
    assert res["lf0_rmse_cents"].tolist() == [0.0, 0.0]
    assert (res["n_voiced"] > 5).all()
    # each utterance keeps the framing of its own single call
    one = M.compare_wavs(w[1:, :lens[1]], None, w[1:, :lens[1]], None, stft, align="none")
    assert one["path_len"].tolist() == [1 + lens[1] // hop] and one["n_voiced"].tolist() == [res["n_voiced"][1].item()]
    # a shifted pitch is measured: one octave down = 1200 cents on every pair voiced in both
    pr = torch.full((1, 30), 200.0, device=DEV)
    mel = torch.randn(1, 80, 30, device=DEV)
    octave = M.compare_mels(mel, None, mel, None, pr, pr / 2, align="none")
    assert octave["lf0_rmse_cents"].item() == pytest.approx(1200.0, rel=1e-12) and octave["n_voiced"].item() == 30
