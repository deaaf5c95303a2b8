"""GPU: the loudness kernels (csrc/loudness.hip through ctts_amd.loudness) against the float64 restatement of tests/loudness_restate.py
(itself pinned to the standard in tests/test_loudness_restate_cpu.py).

The bar.  |L_kernel - L_64| in LU, and the same for every block of the momentary curve that lies above the absolute gate, must not
exceed FACTOR = 1 times the error of the same chain evaluated in stock float32 (scipy.signal.lfilter on float32 arrays, float64 block
sums) plus FLOOR = 1e-9 LU.  The floor is the arithmetic the kernel and the restatement share: both carry the recursion in double, and a
double recursion with the high pass's double pole at r = 1 - 2 pi 38 / rate holds a relative error of about 2^-53 / (1 - r)^2 = 4e-12 at
48 kHz in y, 1e-11 in a block energy, 4e-11 LU; two evaluations that round differently (fused multiply-adds on the device, the scan of
chunk states) may differ by that much, and 1e-9 leaves a factor of 25.  Printed under -s: kernel err / float32 err / bar.
Worst measured on one MI355X over every case of this file: kernel 8.2e-11 LU (30 Hz + 60 Hz at 48 kHz, momentary curve; 7.0e-11 in L)
where float32 is off by 2.7e-4 LU; typical 1e-12 against 1e-5.  The floor never decided a case, so FACTOR stayed 1.

Everything else is exact: samples at and beyond an utterance's length are guard cells (1e30 / NaN) that must not leak; loudness, gain
and the normalised audio of an utterance are bit-equal alone, in a batch of 3, in a batch of 16 and across calls."""
import math
import os

import numpy as np
import pytest
import torch

from ctts_amd import audio, kernels as K, loudness as LD, preprocess as PP, resample as RS, vocoder as V
from ctts_amd._lib import CttsError
from ctts_amd.configs import get_configs
from tests import hifigan_restate as HR
from tests import loudness_restate as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTOR, FLOOR = 1.0, 1e-9
RATES = [22050, 48000, 16000, 11025]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def speechlike(n, sr, seed):
    """gliding fundamental + 5 harmonics under a syllable envelope, noise in the unvoiced stretches (as tools/bench_resample.py)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    f = 150.0 + 60.0 * np.sin(2 * np.pi * (0.7 + 0.3 * rng.random()) * t + rng.random() * 6) + 30.0 * np.sin(2 * np.pi * 2.3 * t)
    ph = 2 * np.pi * np.cumsum(f) / float(sr)
    x = sum(np.sin(k * ph) / k for k in range(1, 7))
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t + rng.random() * 6)
    voiced = np.sin(2 * np.pi * 1.3 * t + rng.random() * 6) > -0.5
    return np.clip(np.where(voiced, 0.3 * x * env, 0.02 * rng.standard_normal(n)), -1, 1).astype(np.float32)


def noise(n, seed, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def rumble(n, sr):
    """30 Hz + 60 Hz: below and just above the 38 Hz corner, where the high pass's poles do the work"""
    t = np.arange(n) / float(sr)
    return (0.4 * np.sin(2 * np.pi * 30.0 * t) + 0.3 * np.sin(2 * np.pi * 60.0 * t + 1.0)).astype(np.float32)


def guarded(rows, N):
    """[B, N] float32 with the rows left-aligned and 1e30 / NaN alternating at and beyond each row's length: never to be read"""
    host = np.empty((len(rows), N), dtype=np.float32)
    host[:, 0::2] = 1e30
    host[:, 1::2] = np.nan
    for i, r in enumerate(rows):
        host[i, :len(r)] = r
    return host


class Ref:
    """float64 and float32 evaluations of one signal, computed once"""

    def __init__(self, x, rate):
        self.z64 = R.block_energies(x, rate)
        self.z32 = R.block_energies(x, rate, dtype=np.float32)
        self.L64, self.valid = R.gate(self.z64)
        self.L32, _ = R.gate(self.z32)
        with np.errstate(divide="ignore"):
            self.l64, self.l32 = -0.691 + 10 * np.log10(self.z64), -0.691 + 10 * np.log10(self.z32)
        self.audible = self.l64 > R.ABSOLUTE_GATE
        self.bar_L = FACTOR * abs(self.L32 - self.L64) + FLOOR
        self.bar_l = FACTOR * float(np.max(np.abs(self.l32 - self.l64)[self.audible])) + FLOOR


def check(name, x, rate, L, curve, valid):
    ref = Ref(x, rate)
    eL = abs(L - ref.L64)
    el = float(np.max(np.abs(curve[:len(ref.l64)] - ref.l64)[ref.audible]))
    print(f"{name:>28s} @{rate}: L {L:9.4f}  kernel err {eL:.2e} / float32 err {abs(ref.L32 - ref.L64):.2e} / bar {ref.bar_L:.2e};  "
          f"curve {el:.2e} / {ref.bar_l - FLOOR:.2e} / {ref.bar_l:.2e}")
    assert valid == ref.valid == 1
    assert eL <= ref.bar_L and el <= ref.bar_l, (name, rate, eL, ref.bar_L, el, ref.bar_l)
    assert len(ref.l64) == R.n_blocks(len(x), rate) and np.all(np.isneginf(curve[len(ref.l64):]))
    return ref


def measure(rows, rate, N=None):
    N = N or max(len(r) for r in rows)
    lens = [len(r) for r in rows]
    wav = torch.from_numpy(guarded(rows, N)).to(DEV)
    L, valid = LD.integrated_loudness(wav, lens, rate)
    curve = LD.loudness_curve(wav, lens, rate)
    return L.cpu().numpy(), valid.cpu().numpy(), curve.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("rate", RATES)
def test_accuracy_against_float64(rate):
    """A ragged batch of three with guard cells: white noise, the speech-like signal, 30 + 60 Hz.
    Measured (one MI355X), kernel err / float32 err in LU, L then curve: 48000 Hz speech-like 1.0e-12 / 2.8e-5, 9.2e-12 / 6.1e-5;
    48000 Hz 30 + 60 Hz 7.0e-11 / 2.1e-4, 8.2e-11 / 2.7e-4 (the worst case of the file); 16000 Hz 30 + 60 Hz 6.6e-12 / 4.4e-5;
    11025 Hz speech-like 1.8e-14 / 3.1e-5; white noise at 16000 Hz 0 / 1.8e-6."""
    rows = [noise(int(1.37 * rate) + 5, 1), speechlike(int(2.1 * rate) + 1, rate, 2), rumble(int(1.73 * rate), rate)]
    L, valid, curve = measure(rows, rate, N=max(len(r) for r in rows) + 37)
    assert L.dtype == np.float64 and curve.dtype == np.float64 and np.all(np.isfinite(L))
    for i, name in enumerate(("white noise", "speech-like", "30 Hz + 60 Hz")):
        check(name, rows[i], rate, L[i], curve[i], valid[i])


def test_edge_lengths_and_scan_levels():
    """Lengths on every edge of the chunking, read from the wrapper: one block exactly; around a chunk boundary; around a tile (64
    chunks); two tiles plus one; around 257 and 4097 chunks, where the state scan gains its third and fourth level."""
    rate, C = 16000, K.loudness_chunk()
    block, tile = int(math.ceil(0.4 * rate)), 64 * C
    k = block // C + 1
    lens = [block, k * C - 1, k * C, k * C + 1, tile - 1, tile, tile + 1, 2 * tile + 1, block + 1,
            257 * C, 257 * C + 1, 258 * C + 1, 4097 * C + 1, 4098 * C + 1]
    assert min(lens) >= block and tile + 1 >= block
    rows = [noise(n, 100 + i, 0.05) + 0.2 * rumble(n, rate) for i, n in enumerate(lens)]
    L, valid, curve = measure(rows, rate)
    for i, n in enumerate(lens):
        check(f"len {n}", rows[i], rate, L[i], curve[i], valid[i])


@pytest.mark.parametrize("rate", RATES)
def test_one_block_exactly_and_the_cut_block(rate):
    n0 = int(math.ceil(0.4 * rate))
    lens = [n0, int(0.449 * rate), int(0.451 * rate) + 1]
    rows = [noise(n, 7 + i) for i, n in enumerate(lens)]
    L, valid, curve = measure(rows, rate, N=lens[-1] + 3)
    assert [R.n_blocks(n, rate) for n in lens] == [1, 1, 2] and curve.shape[1] == 2
    for i in range(3):
        check(f"len {lens[i]}", rows[i], rate, L[i], curve[i], valid[i])


def test_short_term_curve():
    rate = 22050
    rows = [speechlike(int(4.3 * rate), rate, 5), noise(int(3.05 * rate), 6)]
    wav = torch.from_numpy(guarded(rows, len(rows[0]) + 11)).to(DEV)
    got = LD.loudness_curve(wav, [len(r) for r in rows], rate, window="short_term").cpu().numpy()
    for i, x in enumerate(rows):
        want, f32 = R.short_term(x, rate), R.short_term(x, rate, dtype=np.float32)
        bar = FACTOR * float(np.max(np.abs(f32 - want))) + FLOOR
        err = float(np.max(np.abs(got[i, :len(want)] - want)))
        print(f"short-term row {i}: {len(want)} blocks, kernel err {err:.2e} / float32 err {bar - FLOOR:.2e} / bar {bar:.2e}")
        assert err <= bar and np.all(np.isneginf(got[i, len(want):]))


# ---------------------------------------------------------------------------------------------------------------------- independence
def test_bit_equal_alone_in_a_batch_and_across_calls():
    rate = 22050
    rows = [speechlike(int(1.9 * rate) + 3, rate, 11), noise(int(0.77 * rate), 12), rumble(int(1.2 * rate) + 1, rate)]
    lens = [len(r) for r in rows]

    def run(batch_rows, N):
        wav = torch.from_numpy(guarded(batch_rows, N)).to(DEV)
        out, L, g, v = LD.normalize_loudness(wav, [len(r) for r in batch_rows], rate)
        return out.cpu().numpy(), L.cpu().numpy(), g.cpu().numpy(), v.cpu().numpy()

    three = run(rows, max(lens) + 29)
    again = run(rows, max(lens) + 29)
    others = [noise(int((0.5 + 0.21 * i) * rate), 40 + i, 0.03 * (i + 1)) for i in range(13)]
    sixteen = run(others[:5] + [rows[0]] + others[5:9] + [rows[1], rows[2]] + others[9:], int(3.4 * rate))
    where = [5, 10, 11]
    for a, b in zip(three, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for i, n in enumerate(lens):
        alone = run([rows[i]], n)
        for res, j in ((three, i), (sixteen, where[i])):
            assert alone[1][0].tobytes() == res[1][j].tobytes() and alone[2][0].tobytes() == res[2][j].tobytes() and res[3][j] == 1
            assert np.array_equal(alone[0][0, :n].view(np.uint32), res[0][j, :n].view(np.uint32))
            assert not res[0][j, n:].any()


# ---------------------------------------------------------------------------------------------------------------------- normalisation
def test_normalised_audio():
    rate = 22050
    clicks = np.zeros(int(0.9 * rate), dtype=np.float32)
    clicks[::50] = 0.9                                       # little loudness under a high peak: normalising to -10 LUFS would clip
    rows = [speechlike(int(1.3 * rate), rate, 21), noise(int(0.8 * rate) + 2, 22, 0.4), clicks,
            np.zeros(int(0.6 * rate), dtype=np.float32), noise(int(0.7 * rate), 23, 1e-6)]
    lens = [len(r) for r in rows]
    for N in ((max(lens) + 7) // 4 * 4, (max(lens) + 7) // 4 * 4 + 1):      # a multiple of 4 or not: both store paths
        wav = torch.from_numpy(guarded(rows, N)).to(DEV)
        out, L, gain, valid = LD.normalize_loudness(wav, lens, rate, target=-10.0)
        out, L, gain, valid = out.cpu().numpy(), L.cpu().numpy(), gain.cpu().numpy(), valid.cpu().numpy()
        assert out.dtype == np.float32 and gain.dtype == np.float32
        for i, x in enumerate(rows):
            want, L64, g64, ok = R.normalize(x, rate, -10.0)
            assert valid[i] == ok and not out[i, lens[i]:].any()
            if not ok:
                assert np.isneginf(L[i]) and gain[i] == 1.0 and np.array_equal(out[i, :lens[i]].view(np.uint32), x.view(np.uint32))
                continue
            bar = Ref(x, rate).bar_L
            assert abs(L[i] - L64) <= bar
            tol = (2 * 2.0 ** -24 + math.log(10) / 20 * bar) * np.abs(want)
            assert np.all(np.abs(out[i, :lens[i]].astype(np.float64) - want) <= tol), i
        assert valid.tolist() == [1, 1, 1, 0, 0]
        assert np.max(np.abs(out[2])) <= 1.0 and np.max(np.abs(out[2])) > 0.999 and gain[2] == np.float32(1.0) / np.float32(0.9)
        free = LD.normalize_loudness(wav, lens, rate, target=-10.0, peak_limit=False)[0].cpu().numpy()
        assert np.max(np.abs(free[2])) > 1.0
    # in place
    wav = torch.from_numpy(guarded(rows, N)).to(DEV)
    res = LD.normalize_loudness(wav, lens, rate, target=-10.0, out=wav)[0]
    assert res.data_ptr() == wav.data_ptr() and np.array_equal(res.cpu().numpy(), out)


def test_reaches_the_target():
    rate = 48000
    x = speechlike(int(1.5 * rate), rate, 31)
    out, L, gain, valid = LD.normalize_loudness(torch.from_numpy(x[None]).to(DEV), None, rate)
    L2, _ = R.integrated_loudness(out[0].cpu().numpy().astype(np.float64), rate)
    assert abs(L2 + 22.0) <= Ref(x, rate).bar_L + 20 * math.log10(1 + 2.0 ** -23)      # the gain and each product rounded once to fp32


# ---------------------------------------------------------------------------------------------------------------------- errors
def test_errors():
    rate = 22050
    wav = torch.zeros(3, 9000, device=DEV)
    with pytest.raises(ValueError, match=r"\[1\]"):
        LD.integrated_loudness(wav, [9000, 8819, 8820], rate)
    with pytest.raises(ValueError, match=r"\[0, 2\]"):
        LD.normalize_loudness(wav, [100, 9000, 0], rate)
    with pytest.raises(ValueError):
        LD.loudness_curve(wav, [9000] * 3, rate, window="short_term")         # 3 s blocks
    with pytest.raises(ValueError):
        LD.loudness_curve(wav, [9000] * 3, rate, window="weekly")
    with pytest.raises(ValueError):
        LD.integrated_loudness(wav, [9001] * 3, rate)
    for fn in (LD.integrated_loudness, LD.loudness_curve, LD.normalize_loudness):
        with pytest.raises(CttsError):
            fn(torch.zeros(1, 9000), [9000], rate)
    with pytest.raises(CttsError):
        LD.integrated_loudness(torch.zeros(9000, device=DEV), [9000], rate)
    with pytest.raises(CttsError):
        K.apply_gain(torch.zeros(1, 8), torch.zeros(1, dtype=torch.int32), torch.ones(1))
    with pytest.raises(CttsError):
        PP.process_batch_loudness([torch.zeros(9000)], [3], audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000), get_configs()[0])


# ---------------------------------------------------------------------------------------------------------------------- integration
def test_process_batch_loudness_equals_process_batch_on_restated_audio():
    """mel tolerance: 1e-3 on the log-mel, the bar the model tests put on mels (tests/test_model_gpu.py MEL_TOL); the two inputs differ
    by the rounding of the gain and of one product per sample"""
    stft = audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(DEV)
    pre, _, _ = get_configs()
    pre["preprocessing"]["audio"]["trim_top_db"] = 23
    nph = [9, 6]
    w48 = [torch.from_numpy(0.25 * speechlike(n, 48000, s)).to(DEV) for n, s in ((48000, 41), (39007, 42))]
    got = PP.process_batch_loudness(w48, nph, stft, pre, loudness=-22.0, source_rate=48000)
    lens = [int(w.numel()) for w in w48]
    batch = torch.zeros(2, max(lens), device=DEV)
    for i, w in enumerate(w48):
        batch[i, :lens[i]] = w
    res, res_lens = RS.resample(batch, lens, 48000, 22050)
    restated = []
    for i, n in enumerate(res_lens.tolist()):
        out64, L, g, ok = R.normalize(res[i, :n].cpu().numpy().astype(np.float64), 22050, -22.0)
        assert ok == 1 and abs(R.integrated_loudness(out64, 22050)[0] + 22.0) < 1e-6
        restated.append(torch.from_numpy(out64.astype(np.float32)).to(DEV))
    want = PP.process_batch(restated, nph, stft, pre)
    plain = PP.process_batch(w48, nph, stft, pre, source_rate=48000)
    for g, w, p in zip(got, want, plain):
        assert (g["start"], g["end"], g["duration"]) == (w["start"], w["end"], w["duration"]) == (p["start"], p["end"], p["duration"])
        assert g["mel"].shape == w["mel"].shape and g["duration"] > 20
        assert float(np.max(np.abs(g["mel"] - w["mel"]))) <= 1e-3
        assert float(np.max(np.abs(g["mel"] - p["mel"]))) > 0.05          # the level did change


def test_infer_wavs_loudness_delivers_the_target():
    z, h, sd = HR.load_g17(os.path.join(GOLD, "g17_hifigan_small.npz"))
    g = V.Generator(V.AttrDict(h))
    g.load_state_dict(sd)
    g.eval().to(DEV)
    mel = torch.from_numpy(z["mel"]).to(DEV).repeat(1, 1, 2)                  # 64 frames: 0.74 s, the golden 32 are shorter than a block
    mel_lens = [64, 50]
    plain = V.infer_wavs(g, mel, mel_lens)
    got = V.infer_wavs_loudness(g, mel, mel_lens, loudness=-22.0, sampling_rate=22050)
    q = 1.0 / 32768.0
    for a, b in zip(plain, got):
        assert b.dtype == np.int16 and b.shape == a.shape
        x = b.astype(np.float64) * q
        L, ok = R.integrated_loudness(x, 22050)
        # the cast truncates: every sample moves by less than one step q, which K-weighting amplifies by at most the shelf's 4 dB
        rms = math.sqrt(float(np.mean(R.kweight(x, 22050) ** 2)))
        allowance = 20 * math.log10(1 + 10 ** (4 / 20) * q / rms)
        peak_bound = int(np.max(np.abs(b.astype(np.int32))))
        print(f"infer_wavs_loudness: {len(b)} samples read {L:.4f} LUFS, allowance {allowance:.4f} LU, peak {peak_bound}")
        assert ok == 1 and peak_bound < 32767                               # the peak guard did not act: the target applies
        assert abs(L + 22.0) <= allowance + FLOOR + 20 * math.log10(1 + 2.0 ** -23)      # + the gain rounded once to fp32
