"""GPU: the resampling and peak-normalisation kernels (csrc/resample.hip through ctts_amd.resample) against the float64 restatement of
tests/resample_restate.py (itself checked against scipy.signal.resample_poly in tests/test_resample_restate_cpu.py).

Bars.  Impulses: EXACT - one product per output, y[n] == float32(h)[n M + half - k0 L] * amplitude, 0 where that index does not exist.
Noise and tones: per output |y - y64| <= (T_n + 2) 2^-24 sum_k |h[k] x[k]| with T_n the number of terms of that output - T_n roundings of
the running sum, one of each tap to float32 and one to spare; it holds for any summation order.  Padding exactly 0, lengths exact.
L == M, repeated calls, a row against its own B = 1 call and against a batch large enough to change the launch geometry: bit-equal.
Peak normalisation: equal to the numpy float32 statement on every sample, saturating where the reference's int16 cast wraps."""
import math

import numpy as np
import pytest
import torch

from ctts_amd import audio, kernels as K, preprocess as PP, resample as RS
from ctts_amd._lib import CttsError
from ctts_amd.configs import get_configs
from tests import resample_restate as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def padded(rows, N, seed, fill=None):
    """[B, N] float32 with the rows left-aligned and LOUD noise (or `fill`) at and beyond each row's length: it must never be read"""
    host = np.random.default_rng(seed).uniform(-50.0, 50.0, (len(rows), N)).astype(np.float32) if fill is None else np.full((len(rows), N), fill, np.float32)
    for i, r in enumerate(rows):
        host[i, :len(r)] = r
    return host


def tile_of(L, M, h):
    half = (len(h) - 1) // 2
    return K.resample_tile(L, M, RS.phase_taps(L, half), half)


# ---------------------------------------------------------------------------------------------------------------------- impulses
@pytest.mark.parametrize("zeros", [4, 64])
@pytest.mark.parametrize("a,b", [(48000, 22050), (2, 1), (1, 2), (22050, 48000), (22050, 16000)])      # L/M = 147/320, 1/2, 2/1, 320/147, 320/441
def test_impulse_response_is_the_filter_exactly(a, b, zeros):
    L, M, h = RS.resample_filter(a, b, zeros=zeros)
    assert (L, M) == R.design(a, b, zeros)[:2]
    h32, half = h.astype(np.float32), (len(h) - 1) // 2
    N = 700
    rows, where = [], []
    for i, amp in enumerate((1.0, 2.0 ** -3)):
        for jdx, pick in enumerate(("first", "second", "mid", "last")):
            n = N - 3 * (4 * i + jdx)                           # ragged: every row its own length, one impulse per row (supports cannot overlap)
            k0 = {"first": 0, "second": 1, "mid": n // 2 + 1, "last": n - 1}[pick]
            x = np.zeros(n, dtype=np.float32)
            x[k0] = amp
            rows.append(x)
            where.append((k0, amp))
    lens = [len(r) for r in rows]
    out, out_lens = RS.resample(torch.from_numpy(padded(rows, N, 1)).to(DEV), dev_i32(lens), a, b, zeros=zeros)
    got = out.cpu().numpy()
    assert got.shape == (len(rows), R.out_len(N, L, M)) and out_lens.tolist() == [R.out_len(n, L, M) for n in lens]
    for bi, (k0, amp) in enumerate(where):
        olen = R.out_len(lens[bi], L, M)
        idx = np.arange(olen, dtype=np.int64) * M + half - k0 * L
        ok = (idx >= 0) & (idx < len(h32))
        want = np.where(ok, h32[np.clip(idx, 0, len(h32) - 1)], np.float32(0)) * np.float32(amp)
        assert ok.any() and want.dtype == np.float32
        assert np.array_equal(got[bi, :olen], want), (a, b, zeros, bi, k0, int(np.flatnonzero(got[bi, :olen] != want)[0]))
        assert np.all(got[bi, olen:] == 0)


# ---------------------------------------------------------------------------------------------------------------------- noise and tones
CONFIGS = [(48000, 22050, "kaiser_best"), (48000, 22050, "kaiser_fast"), (22050, 48000, "kaiser_best"), (22050, 44100, "kaiser_best"),
           (44100, 22050, "kaiser_fast"), (22050, 16000, "kaiser_best")]


def len_for(o, L, M):
    """the shortest input whose output has at least o samples (exactly o whenever L <= M)"""
    n = max(1, (o - 1) * M // L)
    while R.out_len(n, L, M) < o:
        n += 1
    return n


@pytest.fixture(scope="module")
def signals():
    cache = {}

    def make(a, b, quality):
        if (a, b, quality) in cache:
            return cache[a, b, quality]
        L, M, h = RS.resample_filter(a, b, quality)
        tile = tile_of(L, M, h)
        assert tile > 0 and tile % L == 0
        out_lens = [1, 2, tile - 1, tile, tile + 1, 2 * tile + 1]
        lens = [len_for(o, L, M) for o in out_lens] + [1, max(M - 1, 1), M, M + 1]
        if L <= M:
            assert [R.out_len(n, L, M) for n in lens[:6]] == out_lens
        rng = np.random.default_rng(a + b + len(quality))
        rows = []
        for i, n in enumerate(lens):
            t = np.arange(n) / float(a)
            tone = 0.4 * np.sin(2 * np.pi * 440.0 * t + i) + 0.3 * np.sin(2 * np.pi * 0.31 * a * t)       # one tone in the band, one near the edge
            rows.append((rng.standard_normal(n) if i % 2 == 0 else tone + 0.01 * rng.standard_normal(n)).astype(np.float32))
        ref = [R.resample(r.astype(np.float64), h, L, M) for r in rows]
        f32 = [R.resample_f32(r, h, L, M) for r in rows]
        cache[a, b, quality] = (L, M, h, tile, rows, ref, f32)
        return cache[a, b, quality]
    return make


@pytest.mark.parametrize("a,b,quality", CONFIGS)
def test_noise_and_tones_within_the_derived_bound_of_float64(signals, a, b, quality):
    L, M, h, tile, rows, ref, f32 = signals(a, b, quality)
    lens = [len(r) for r in rows]
    N = max(lens) + 37
    out, out_lens = RS.resample(torch.from_numpy(padded(rows, N, 2)).to(DEV), dev_i32(lens), a, b, quality)
    got = out.cpu().numpy()
    want_lens = [R.out_len(n, L, M) for n in lens]
    assert got.shape == (len(rows), R.out_len(N, L, M)) and out_lens.tolist() == want_lens
    worst = (0.0, 0.0, 0.0)
    for bi, (y64, mag, terms) in enumerate(ref):
        olen = want_lens[bi]
        assert len(y64) == olen and np.all(got[bi, olen:] == 0)
        bound = (terms + 2) * 2.0 ** -24 * mag
        err = np.abs(got[bi, :olen].astype(np.float64) - y64)
        e32 = np.abs(f32[bi].astype(np.float64) - y64)
        i = int(np.argmax(err / np.maximum(bound, 1e-300)))
        if err[i] / max(bound[i], 1e-300) >= worst[0]:
            worst = (err[i] / max(bound[i], 1e-300), err[i], bound[i])
        print(f"{a}->{b} {quality} len {lens[bi]:6d} -> {olen:6d}: kernel max err {err.max():.3e}, float32 restatement {e32.max():.3e}, "
              f"bound there {bound[int(np.argmax(err))]:.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound), (a, b, quality, lens[bi], i, err[i], bound[i])
    print(f"{a}->{b} {quality}: tile {tile}, worst err / bound {worst[0]:.3f} ({worst[1]:.3e} against {worst[2]:.3e})")


def test_ragged_batch_of_five_ignores_what_lies_beyond_the_lengths(signals):
    a, b, quality = 48000, 22050, "kaiser_fast"
    L, M, h, tile, rows, ref, _ = signals(a, b, quality)
    pick = [9, 3, 6, 0, 4]                                      # lengths M + 1, tile, 1 (noise), 1, tile + 1 outputs
    sel = [rows[i] for i in pick]
    lens = [len(r) for r in sel]
    N = max(lens) + 5
    x1 = torch.from_numpy(padded(sel, N, 3)).to(DEV)
    x2 = torch.from_numpy(padded(sel, N, 4, fill=np.float32("nan"))).to(DEV)          # NaN beyond the lengths: a read would poison the row
    o1, l1 = RS.resample(x1, dev_i32(lens), a, b, quality)
    o2, l2 = RS.resample(x2, lens, a, b, quality)               # host-given lengths take the same path
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and l1.tolist() == [R.out_len(n, L, M) for n in lens]
    got = o1.cpu().numpy()
    for bi, i in enumerate(pick):
        y64, mag, terms = ref[i]
        assert np.all(np.abs(got[bi, :len(y64)] - y64) <= (terms + 2) * 2.0 ** -24 * mag) and np.all(got[bi, len(y64):] == 0)
    # device-given lengths are clamped to [0, N]
    o3, l3 = RS.resample(x1[:2], dev_i32([-4, N + 100]), a, b, quality)
    assert l3.tolist() == [0, R.out_len(N, L, M)] and np.all(o3[0].cpu().numpy() == 0)
    with pytest.raises(ValueError):
        RS.resample(x1, [N + 1] + lens[1:], a, b, quality)
    with pytest.raises(ValueError):
        RS.resample(x1, lens[1:], a, b, quality)


# ---------------------------------------------------------------------------------------------------------------------- identities
def test_equal_rates_copy_bitwise():
    rng = np.random.default_rng(5)
    rows = [rng.standard_normal(n).astype(np.float32) for n in (1, 255, 256, 257, 1000)]
    rows[3][:4] = [-0.0, 0.0, np.float32(1e-45), -np.float32(3e38)]
    lens = [len(r) for r in rows]
    host = padded(rows, 1003, 6)
    out, out_lens = RS.resample(torch.from_numpy(host).to(DEV), dev_i32(lens), 22050, 22050)
    got = out.cpu().numpy()
    assert got.shape == host.shape and out_lens.tolist() == lens
    for bi, r in enumerate(rows):
        assert np.array_equal(got[bi, :lens[bi]].view(np.uint32), r.view(np.uint32))
        assert np.all(got[bi, lens[bi]:].view(np.uint32) == 0)
    again, _ = RS.resample(torch.from_numpy(host).to(DEV), lens, 48000, 48000, "kaiser_fast")
    assert torch.equal(again, out)


def test_repeatable_and_independent_of_batch_and_geometry(signals):
    a, b, quality = 48000, 22050, "kaiser_best"
    L, M, h, tile, rows, _, _ = signals(a, b, quality)
    sel = [rows[i] for i in (4, 9, 2, 1)]                       # tile + 1 outputs, M + 1 samples, tile - 1 outputs, 2 outputs
    lens = [len(r) for r in sel]
    N = max(lens) + 11
    x = torch.from_numpy(padded(sel, N, 7)).to(DEV)
    o1, l1 = RS.resample(x, dev_i32(lens), a, b, quality)
    o2, l2 = RS.resample(x, dev_i32(lens), a, b, quality)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)          # two calls
    for bi, n in enumerate(lens):
        olen = R.out_len(n, L, M)
        alone, la = RS.resample(x[bi:bi + 1].contiguous(), dev_i32([n]), a, b, quality)          # B = 1, same padded width
        assert torch.equal(alone[0], o1[bi]) and la.tolist() == [olen]
        cut, lc = RS.resample(x[bi:bi + 1, :n].contiguous(), None, a, b, quality)                # B = 1, its own width: another grid
        assert cut.shape == (1, olen) and torch.equal(cut[0], o1[bi, :olen]) and lc.tolist() == [olen]
    # a batch large enough that the kernel stops splitting a tile's phases over several workgroups
    n = lens[1]
    many = x[1:2, :n + 3].repeat(600, 1).contiguous()
    om, _ = RS.resample(many, dev_i32([n] * 600), a, b, quality)
    assert torch.equal(om, o1[1, :om.shape[1]].expand_as(om))


# ---------------------------------------------------------------------------------------------------------------------- peak normalisation
def test_peak_normalize_is_the_numpy_statement_and_saturates():
    rng = np.random.default_rng(11)
    pos = (0.37 * rng.standard_normal(5000)).astype(np.float32)
    pos[1234] = np.abs(pos).max() * np.float32(1.25)            # the peak is positive: v = +32768 there, the reference's cast wraps
    neg = (0.02 * rng.standard_normal(4097)).astype(np.float32)
    neg[7] = -np.abs(neg).max() * np.float32(1.5)               # the peak is negative: -32768 exactly
    tiny = (1e-30 * rng.standard_normal(300)).astype(np.float32)
    one = np.array([-0.25], dtype=np.float32)
    zero = np.zeros(777, dtype=np.float32)
    rows = [pos, neg, tiny, one, zero]
    lens = [len(r) for r in rows]
    N = 5000 + 96
    host = padded(rows, N, 12)                                  # +-50 beyond the lengths: must not move the peak
    x = torch.from_numpy(host).to(DEV)
    out, valid, q16 = RS.peak_normalize(x, dev_i32(lens), return_int16=True)
    got, gq = out.cpu().numpy(), q16.cpu().numpy()
    assert valid.tolist() == [1, 1, 1, 1, 0] and gq.dtype == np.int16
    for bi, r in enumerate(rows[:4]):
        v, q, f, ref, wraps = R.peak_normalize(r)
        n = lens[bi]
        assert np.array_equal(gq[bi, :n], q) and np.array_equal(got[bi, :n], f), bi
        same = ~wraps
        assert np.array_equal(gq[bi, :n][same], ref[same])      # the reference's own cast everywhere it is defined
        assert np.all(gq[bi, :n][wraps] == 32767) and np.all(ref[wraps] == -32768)
        assert np.all(got[bi, n:] == 0) and np.all(gq[bi, n:] == 0)
    assert R.peak_normalize(pos)[4].sum() == 1 and gq[0, 1234] == 32767 and got[0, 1234] == np.float32(32767 / 32768)
    assert gq[1, 7] == -32768 and got[1, 7] == -1.0 and not R.peak_normalize(neg)[4].any()
    assert np.all(got[4] == 0) and np.all(gq[4] == 0)
    # another max_wav_value, host lengths, no int16 wanted; and twice the same
    out2, valid2 = RS.peak_normalize(x, lens, max_wav_value=20000.0)
    g2 = out2.cpu().numpy()
    for bi, r in enumerate(rows[:4]):
        assert np.array_equal(g2[bi, :lens[bi]], R.peak_normalize(r, 20000.0)[2]), bi
    assert torch.equal(RS.peak_normalize(x, lens, max_wav_value=20000.0)[0], out2) and valid2.tolist() == [1, 1, 1, 1, 0]
    o0, v0 = RS.peak_normalize(x[:2], dev_i32([0, -3]))
    assert v0.tolist() == [0, 0] and np.all(o0.cpu().numpy() == 0)


# ---------------------------------------------------------------------------------------------------------------------- process_batch
def speechlike(n, sr, seed, lead, trail):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    f = 140.0 + 40.0 * np.sin(2 * np.pi * 0.9 * t + seed) + 20.0 * np.sin(2 * np.pi * 2.3 * t)
    ph = 2 * np.pi * np.cumsum(f) / float(sr)
    x = 0.3 * sum(np.sin(k * ph) / k for k in range(1, 6)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t + seed))
    y = 1e-4 * rng.standard_normal(n)
    y[lead:n - trail] = x[lead:n - trail]
    return np.clip(y, -1, 1).astype(np.float32)


def test_process_batch_resamples_first_when_given_a_source_rate():
    stft = audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(DEV)
    pre, _, _ = get_configs()
    pre["preprocessing"]["audio"]["trim_top_db"] = 23
    nph = [11, 7, 15]
    w48 = [torch.from_numpy(speechlike(n, 48000, s, lead, trail)).to(DEV) for n, s, lead, trail in
           ((48000, 1, 6500, 5400), (43571, 2, 3900, 8900), (53503, 3, 10900, 2600))]
    out = PP.process_batch(w48, nph, stft, pre, source_rate=48000)
    lens = [int(w.numel()) for w in w48]
    batch = torch.zeros(3, max(lens), device=DEV)
    for i, w in enumerate(w48):
        batch[i, :lens[i]] = w
    res, res_lens = RS.resample(batch, lens, 48000, 22050)
    w22 = [res[i, :n].clone() for i, n in enumerate(res_lens.tolist())]
    assert [int(w.numel()) for w in w22] == [math.ceil(n * 147 / 320) for n in lens]
    manual = PP.process_batch(w22, nph, stft, pre)
    same_rate = PP.process_batch(w22, nph, stft, pre, source_rate=22050)
    for o, m, s in zip(out, manual, same_rate):
        assert set(o) == set(m) == set(s)
        assert 40 < o["duration"] < 110 and o["valid"] == 1 and 0 < o["start"] < o["end"] <= math.ceil(53503 * 147 / 320)
        for k, v in m.items():
            assert np.array_equal(v, o[k]) and np.array_equal(v, s[k]), k
    fast = PP.process_batch(w48, nph, stft, pre, source_rate=48000, resample_quality="kaiser_fast")
    assert fast[0]["mel"].shape[1] == 80 and not np.array_equal(fast[0]["mel"], out[0]["mel"])


def test_cpu_tensors_raise():
    with pytest.raises(CttsError):
        RS.resample(torch.zeros(1, 100), [100], 48000, 22050)
    with pytest.raises(CttsError):
        RS.resample(torch.zeros(1, 100), dev_i32([100]), 48000, 22050)
    with pytest.raises(CttsError):
        RS.peak_normalize(torch.zeros(1, 100), [100])
    with pytest.raises(CttsError):
        RS.resample(torch.zeros(100, device=DEV), [100], 48000, 22050)       # not a [B, N] batch
    with pytest.raises(ValueError):
        RS.resample(torch.zeros(1, 100, device=DEV), [100], 48000, 22051)    # refused on the host, before any launch
