"""GPU: the waveform metrics (csrc/wavmetrics.hip through ctts_amd.metrics and ctts_amd.kernels) against the float64 restatement of
tests/wavmetrics_restate.py (itself pinned in tests/test_wavmetrics_restate_cpu.py) on the case table of tests/wavmetrics_inputs.py.

Counts (frames, kept, segments, STFT frames) and the NaN / inf pattern must EQUAL the restatement's on every case; the CPU test shows
that no case has a frame within 1e-6 dB of its keep threshold, and this file shows the same for the resampled audio it restates.

The bar on every value (STOI, ESTOI, SI-SDR in dB, sc, log_mag, lsd_db):  |kernel - f64| <= FACTOR |f32 evaluation - f64| + FLOOR with
FACTOR = 1 and FLOOR = 1e-9.  The floor is what the kernels and the restatement share: both are double evaluations of one definition
that round in different orders (radix-2 transform of x + i y in LDS against pocketfft's real transform, fused multiply-adds, tree sums
against pairwise sums).  A double transform of 512 .. 2048 points is off by about log2(n) 2^-53 = 1e-15 of the frame's largest bin;
a band or bin 60 dB below that bin (the table's speech-like signals span less) carries that error at 1e-12 relative, and STOI / ESTOI
(correlations of normalised rows), sc and the two log distances move by no more than the relative error of what they are made of.
SI-SDR from the five sums loses ||y||^2 / ||y - t||^2 in the residual: 2^-52 * 1e3 at the table's best case, 30 dB, which is 1e-12 dB.
1e-9 leaves three orders over that and sits two to four orders under the float32 evaluation, so it cannot hide a float32-sized fault.
Printed under -s: kernel err / float32 err / bar for every value.
MEASURED (one MI355X, every case of this file), worst kernel err / float32 err of the same case, and the case that decided:
  stoi 4.1e-14 / 3.5e-6 (speech-like 0 dB)       estoi 7.5e-14 / 2.0e-6 (speech-like -10 dB)     si_sdr 9.2e-13 dB / 1.3e-6 (speech-like +30 dB)
  sc 2.7e-12 / 1.2e-3 (all-zero reference, where sc is 1e3)     log_mag 1.8e-15 / 8.6e-7     lsd_db 2.8e-14 / 5.0e-6 (both: all-zero reference)
The floor never decided a case (the smallest float32 error with a kernel error above 0 was 7.5e-10), so FACTOR stayed 1.

For rate != 10000 the expected value is the restatement applied to the device's own resampled audio (the resampler has its own tests;
an end-to-end float64 chain would let one rounding of the resampler flip a keep decision).  Samples at and beyond every length, and
every output and workspace word of the raw C-ABI call, start as guard cells (1e30 / NaN): none may leak.  Each utterance's results are
bit-equal alone, in a batch of 3, in a batch of 16 and across two calls."""
import ctypes
import math

import numpy as np
import pytest
import torch

from ctts_amd import _lib, kernels as K, metrics as M, resample as RS
from ctts_amd._lib import CttsError
from tests import wavmetrics_inputs as I
from tests import wavmetrics_restate as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTOR, FLOOR = 1.0, 1e-9
VALUES = ("stoi", "estoi", "si_sdr", "sc", "log_mag", "lsd_db")
WORST = {}


def guarded(rows, N):
    """[B, N] float32 with the rows left-aligned and 1e30 / NaN alternating at and beyond each row's length: never to be read"""
    host = np.empty((len(rows), N), dtype=np.float32)
    host[:, 0::2] = 1e30
    host[:, 1::2] = np.nan
    for i, r in enumerate(rows):
        host[i, :len(r)] = r
    return host


def restate(x, y, dtype):
    s = R.stoi(x, y, dtype=dtype)
    m = R.mr_stft_distance(x, y, dtype=dtype)
    return {"stoi": s["stoi"], "estoi": s["estoi"], "frames": s["frames"], "kept": s["kept"], "segments": s["segments"],
            "si_sdr": R.si_sdr(x, y, dtype=dtype), "sc": m["sc"], "log_mag": m["log_mag"], "lsd_db": m["lsd_db"], "mr_frames": m["frames"]}


def stoi_only(x, y, dtype):
    s = R.stoi(x, y, dtype=dtype)
    return {k: s[k] for k in ("stoi", "estoi", "frames", "kept", "segments")}


def same_special(a, b):
    """NaN where NaN, the same infinity where infinite"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isinf(a), a, 0), np.where(np.isinf(b), b, 0))


def check(name, got, want, f32, keys=VALUES):
    for key in ("frames", "kept", "segments", "mr_frames"):
        if key in want:
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), (name, key, got[key], want[key])
    for key in keys:
        g, w, f = (np.atleast_1d(np.asarray(v[key], dtype=np.float64)) for v in (got, want, f32))
        assert same_special(g, w), (name, key, g, w)
        fin = np.isfinite(w)
        if not fin.any():
            print(f"{name:>28s} {key:>8s}: {w.tolist()}")
            continue
        assert np.all(np.isfinite(f[fin])), (name, key, f)
        err, e32 = np.abs(g - w)[fin], np.abs(f - w)[fin]
        bar = FACTOR * e32 + FLOOR
        print(f"{name:>28s} {key:>8s}: kernel err {err.max():.2e} / float32 err {e32.max():.2e} / bar {bar.min():.2e}")
        if err.max() >= WORST.get(key, (-1.0,))[0]:
            WORST[key] = (float(err.max()), float(e32.max()), name)
        assert np.all(err <= bar), (name, key, g, w, f)


def row(res, i):
    return {k: v[i].cpu().numpy() for k, v in res.items()}


def run(cases, rate, pad=41):
    N = max(len(c[1]) for c in cases) + pad
    ref = torch.from_numpy(guarded([c[1] for c in cases], N)).to(DEV)
    syn = torch.from_numpy(guarded([c[2] for c in cases], N)).to(DEV)
    return ref, syn, [len(c[1]) for c in cases]


# ---------------------------------------------------------------------------------------------------------------------- accuracy
def test_every_case_at_10_khz_against_float64():
    cases = I.cases_10k()
    ref, syn, lens = run(cases, 10000)
    got = M.waveform_metrics(ref, syn, lens, 10000)
    assert got["stoi"].dtype == torch.float64 and got["segments"].dtype == torch.int32 and got["sc"].shape == (len(cases), 3)
    seen_nan = seen_val = 0
    for i, (name, x, y) in enumerate(cases):
        want = restate(x, y, np.float64)
        check(name, row(got, i), want, restate(x, y, np.float32))
        seen_nan += math.isnan(want["stoi"])
        seen_val += not math.isnan(want["stoi"])
    assert seen_nan >= 7 and seen_val >= 9
    print("worst:", WORST)
    # the single-metric entry points return the same bits; lengths as a device tensor
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for ext, key in ((False, "stoi"), (True, "estoi")):
        s = M.stoi(ref, syn, lens_d, 10000, extended=ext)
        assert torch.equal(s["stoi"].view(torch.int64), got[key].view(torch.int64)) and torch.equal(s["kept"], got["kept"])
    assert torch.equal(M.si_sdr(ref, syn, lens_d).view(torch.int64), got["si_sdr"].view(torch.int64))
    mr = M.mr_stft_distance(ref, syn, lens_d)
    assert torch.equal(mr["lsd_db"].view(torch.int64), got["lsd_db"].view(torch.int64)) and torch.equal(mr["frames"], got["mr_frames"])
    summary = M.summarize_waveform(got)
    finite = np.array([restate(x, y, np.float64)["stoi"] for _, x, y in cases])
    assert summary["stoi"]["count"] == int((~np.isnan(finite)).sum()) and abs(summary["stoi"]["mean"] - np.nanmean(finite)) <= 1e-9
    assert len(summary["sc"]["mean"]) == 3 and "frames" not in summary


@pytest.mark.parametrize("rate", [c[0] for c in I.RATE_CASES])
def test_other_rates_against_float64_on_the_device_resampled_audio(rate):
    cases = I.cases_rate(rate)
    ref, syn, lens = run(cases, rate)
    got = M.waveform_metrics(ref, syn, lens, rate)
    r10, lens10 = RS.resample(ref, lens, rate, 10000, "kaiser_best")
    s10, _ = RS.resample(syn, lens, rate, 10000, "kaiser_best")
    r10, s10, lens10 = r10.cpu().numpy(), s10.cpu().numpy(), lens10.cpu().numpy()
    for i, (name, x, y) in enumerate(cases):
        n = int(lens10[i])
        assert n == -(-len(x) * 10000 // rate) and n <= 30000
        xr, yr = r10[i, :n], s10[i, :n]
        assert R.threshold_margin_db(xr) > 1e-6, name               # the restated input is a fair one
        g = row(got, i)
        check(name, g, stoi_only(xr, yr, np.float64), stoi_only(xr, yr, np.float32), keys=("stoi", "estoi"))
        want = restate(x, y, np.float64)                            # SI-SDR and the STFT distances are taken at the input rate
        f32 = restate(x, y, np.float32)
        check(name, {k: g[k] for k in ("si_sdr", "sc", "log_mag", "lsd_db", "mr_frames")},
              {k: want[k] for k in ("si_sdr", "sc", "log_mag", "lsd_db", "mr_frames")}, f32, keys=("si_sdr", "sc", "log_mag", "lsd_db"))
        assert 0.3 < g["stoi"] < 1.0


def test_other_resolutions_and_a_short_window():
    name, x, y = I.cases_10k()[9]
    assert len(x) == 20000
    res = ((512, 64, 512), (1024, 300, 1000), (2048, 512, 2048), (2048, 1000, 7))
    ref, syn, lens = run([(name, x, y), (name, x[:1999], y[:1999])], 10000)
    got = M.mr_stft_distance(ref, syn, lens, res)
    for i, n in enumerate(lens):
        want, f32 = R.mr_stft_distance(x[:n], y[:n], res), R.mr_stft_distance(x[:n], y[:n], res, dtype=np.float32)
        g = row(got, i)
        g["mr_frames"], want["mr_frames"] = g["frames"], want["frames"]
        check(f"resolutions, len {n}", {k: v for k, v in g.items() if k != "frames"}, {k: v for k, v in want.items() if k != "frames"}, f32,
              keys=("sc", "log_mag", "lsd_db"))
    assert math.isnan(float(got["sc"][1, 2])) and int(got["frames"][1, 2]) == 0


# ---------------------------------------------------------------------------------------------------------------------- raw C ABI
def test_raw_abi_writes_every_output_over_guard_cells():
    cases = [I.cases_10k()[i] for i in (1, 6, 9, 16, 18)]           # 255 samples, one segment, 20000, the hole, the all-zero reference
    ref, syn, lens = run(cases, 10000, pad=3)
    B, N = ref.shape
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    win = torch.from_numpy(M.stoi_window()).to(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def guard(n, dtype):
        t = torch.empty(n, dtype=dtype, device=DEV)
        if dtype == torch.int32:
            t.fill_(-7)
        else:
            t[0::2] = 1e30
            t[1::2] = float("nan")
        return t
    nbytes = lib.ctts_stoi_workspace_bytes(B, N)
    assert nbytes > 0 and lib.ctts_stoi_workspace_bytes(B, 128 * K.stoi_max_frames() + 256) == 0
    ws, d, e, counts = guard(nbytes // 8, torch.float64), guard(B, torch.float64), guard(B, torch.float64), guard(3 * B, torch.int32)
    assert lib.ctts_stoi(ref.data_ptr(), syn.data_ptr(), lens_d.data_ptr(), win.data_ptr(), d.data_ptr(), e.data_ptr(), counts.data_ptr(), B, N,
                         ws.data_ptr(), stream) == 0
    sd_ws, sd = guard(lib.ctts_si_sdr_workspace_bytes(B, N) // 8, torch.float64), guard(B, torch.float64)
    assert lib.ctts_si_sdr(ref.data_ptr(), syn.data_ptr(), lens_d.data_ptr(), sd.data_ptr(), B, N, sd_ws.data_ptr(), stream) == 0
    n_fft, hop, wn = 1024, 120, 600
    mw = torch.from_numpy(M.mr_stft_window(wn)).to(DEV)
    mr_ws, mr, fr = guard(lib.ctts_mr_stft_workspace_bytes(B, N, hop, wn) // 8, torch.float64), guard(3 * B, torch.float64), guard(B, torch.int32)
    assert lib.ctts_mr_stft(ref.data_ptr(), syn.data_ptr(), lens_d.data_ptr(), mw.data_ptr(), mr.data_ptr(), fr.data_ptr(), B, N, n_fft, hop, wn,
                            mr_ws.data_ptr(), stream) == 0
    counts, mr = counts.view(B, 3).cpu().numpy(), mr.view(B, 3).cpu().numpy()
    for i, (name, x, y) in enumerate(cases):
        want, f32 = restate(x, y, np.float64), restate(x, y, np.float32)
        w1, f1 = R.stft_distance(x, y, n_fft, hop, wn), R.stft_distance(x, y, n_fft, hop, wn, dtype=np.float32)
        got = {"stoi": d[i].item(), "estoi": e[i].item(), "si_sdr": sd[i].item(), "frames": counts[i, 0], "kept": counts[i, 1],
               "segments": counts[i, 2], "sc": mr[i, 0], "log_mag": mr[i, 1], "lsd_db": mr[i, 2], "mr_frames": fr[i].item()}
        want.update(sc=w1[0], log_mag=w1[1], lsd_db=w1[2], mr_frames=w1[3])
        f32.update(sc=f1[0], log_mag=f1[1], lsd_db=f1[2])
        check("raw " + name, got, want, f32)
    # N below one frame: the call still writes every output
    d2, e2, c2 = guard(B, torch.float64), guard(B, torch.float64), guard(3 * B, torch.int32)
    short = torch.zeros(B, 200, device=DEV)
    ws2 = guard(max(lib.ctts_stoi_workspace_bytes(B, 200) // 8, 1), torch.float64)
    assert lib.ctts_stoi(short.data_ptr(), short.data_ptr(), lens_d.data_ptr(), win.data_ptr(), d2.data_ptr(), e2.data_ptr(), c2.data_ptr(), B, 200,
                         ws2.data_ptr(), stream) == 0
    assert torch.isnan(d2).all() and torch.isnan(e2).all() and not c2.any()
    # the typed wrappers give the same bits
    kd, ke, kc = K.stoi(ref, syn, lens_d, win)
    assert torch.equal(kd.view(torch.int64), d.view(torch.int64)) and torch.equal(ke.view(torch.int64), e.view(torch.int64))
    assert np.array_equal(kc.cpu().numpy(), counts)
    assert torch.equal(K.si_sdr(ref, syn, lens_d).view(torch.int64), sd.view(torch.int64))


# ---------------------------------------------------------------------------------------------------------------------- independence
def test_bit_equal_alone_in_a_batch_and_across_calls():
    rate = 16000
    rows = [I.cases_rate(16000)[0], (None, I.noise(9001, 50), I.noise(9001, 51)), I.cases_10k()[16]]
    rows = [(None, x, y) for _, x, y in rows]
    others = [(None, I.noise(3000 + 1777 * i, 60 + i, 0.02 * (i + 1)), I.noise(3000 + 1777 * i, 80 + i)) for i in range(13)]

    def go(cases, pad):
        ref, syn, lens = run(cases, rate, pad)
        return {k: v.cpu().numpy() for k, v in M.waveform_metrics(ref, syn, lens, rate).items()}

    def bits(a):
        return np.ascontiguousarray(a).tobytes()
    three, again = go(rows, 29), go(rows, 29)
    sixteen = go(others[:5] + [rows[0]] + others[5:9] + [rows[1], rows[2]] + others[9:], 1003)
    where = [5, 10, 11]
    for k in three:
        assert bits(three[k]) == bits(again[k]), k
    assert np.isfinite(three["stoi"]).all() and np.isfinite(three["lsd_db"]).all()
    for i in range(3):
        alone = go([rows[i]], 0)
        for k in alone:
            assert bits(alone[k][0]) == bits(three[k][i]) == bits(sixteen[k][where[i]]), (k, i)


# ---------------------------------------------------------------------------------------------------------------------- sanity
def test_stoi_of_a_signal_with_itself_is_one_and_falls_with_the_snr():
    x = I.speechlike(20000, 10000, 2)
    ys = [x] + [I.mix(x, snr, 300) for snr in I.SNRS_DB]
    ref = torch.from_numpy(np.stack([x] * len(ys))).to(DEV)
    syn = torch.from_numpy(np.stack(ys)).to(DEV)
    got = M.waveform_metrics(ref, syn, None, 10000)
    for key in ("stoi", "estoi"):
        v = got[key].cpu().numpy()
        print(key, v)
        assert abs(v[0] - 1.0) <= FLOOR and 1.0 > v[1] > v[2] > v[3] > v[4] > 0.0
    sd = got["si_sdr"].cpu().numpy()
    # the noise is not orthogonal to x: <n,x> / <x,x> is about 10^(-snr/20) / sqrt(20000), 0.2 dB at -10 dB
    assert np.isposinf(sd[0]) and np.all(np.abs(sd[1:] - np.array(I.SNRS_DB)) < 1.0)
    assert float(got["sc"][0].abs().max()) <= FLOOR and float(got["lsd_db"][0].abs().max()) <= FLOOR


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    a = torch.zeros(2, 5000, device=DEV)
    for fn in (lambda r, s: M.stoi(r, s, None, 10000), lambda r, s: M.si_sdr(r, s, None), lambda r, s: M.mr_stft_distance(r, s, None),
               lambda r, s: M.waveform_metrics(r, s, None, 10000)):
        with pytest.raises(CttsError):
            fn(torch.zeros(2, 5000), torch.zeros(2, 5000))
        with pytest.raises(CttsError):
            fn(a, torch.zeros(2, 5000))
        with pytest.raises(CttsError):
            fn(a, torch.zeros(2, 4999, device=DEV))
    for res in (((256, 64, 256),), ((512, 50, 513),), ((1024, 0, 600),), ((1000, 100, 400),), ((512, 50),), ()):
        with pytest.raises(CttsError):
            M.mr_stft_distance(a, a, None, res)
    with pytest.raises(CttsError):
        M.stoi(a, a, [5000, 5001], 10000)
    with pytest.raises(CttsError):
        K.mr_stft(a, a, torch.zeros(2, dtype=torch.int32, device=DEV), torch.ones(600, device=DEV), 1024, 120)      # a float32 window
    limit = 128 * (K.stoi_max_frames() - 1) + 256 + 127
    assert K.stoi_max_frames() >= 4687
    long = torch.zeros(1, limit + 1, device=DEV)
    with pytest.raises(CttsError, match="frames"):
        M.stoi(long, long, None, 10000)
    with pytest.raises(CttsError, match="frames"):
        K.stoi(long, long, torch.zeros(1, dtype=torch.int32, device=DEV), torch.from_numpy(M.stoi_window()).to(DEV))
    ok = M.stoi(long[:, :limit], long[:, :limit], [300], 10000)     # the limit itself is served
    assert int(ok["frames"][0]) == 1 and int(ok["segments"][0]) == 0
