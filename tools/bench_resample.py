"""Audio resampling on the device (csrc/resample.hip through ctts_amd.resample) against the stock-torch polyphase formulation on the same
device and scipy on the host, timed in the same run.  Prints ONE JSON line.

Batch: the canonical 16 speech-like utterances (synthetic.make_batch()'s mel lengths capped at 1024; 256 samples per frame at 22.05 kHz),
synthesised at 48 kHz for the two 48000 -> 22050 cases and at 22.05 kHz for 22050 -> 48000.  Timing: warm-up, then the median over HIP
events around back-to-back calls (tools/bench_pitch_features.timed).  Reported per case: time per call, input samples / s, seconds of
audio per second, achieved bytes / s counted as 4 (N_in + N_out) per call against 8 TB/s, and FMA / s (one per output and filter tap of
its phase) against the fp32 vector peak, so the reader sees which limit the kernel sits under.
Stock torch: `F.conv1d` of the zero-padded batch with an [L, 1, width] kernel - row c holds the taps of output phase c - at stride M,
transposed and flattened: the formulation torchaudio uses, built here from the SAME float32 prototype, its result compared with the
kernel's.  Host: `scipy.signal.resample_poly(x, L, M, window=h / L, padtype="constant")` on the first utterance, when scipy is importable.
The one bar: at kaiser_best on the canonical batch the native call must not be slower than the stock-torch formulation of the same run.
Parity with librosa / resampy is UNPINNED (neither is installed where this project is built).

    python tools/bench_resample.py [--steps 20] [--warmup 3] [--out profiles/resample_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import resample as RS  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402
from bench_pitch_features import timed  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
FP32_VECTOR_FMA_PER_S = 157.3e12 / 2          # MI355X data sheet: 157.3 TFLOP/s fp32 vector


def speechlike(n, sr, seed):
    """gliding fundamental + 5 harmonics under a syllable envelope, noise in the unvoiced stretches (as tools/bench_pitch_features.py)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    f = 150.0 + 60.0 * np.sin(2 * np.pi * (0.7 + 0.3 * rng.random()) * t + rng.random() * 6) + 30.0 * np.sin(2 * np.pi * 2.3 * t)
    ph = 2 * np.pi * np.cumsum(f) / float(sr)
    x = sum(np.sin(k * ph) / k for k in range(1, 7))
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t + rng.random() * 6)
    voiced = np.sin(2 * np.pi * 1.3 * t + rng.random() * 6) > -0.5
    return np.clip(np.where(voiced, 0.3 * x * env, 0.02 * rng.standard_normal(n)), -1, 1).astype(np.float32)


class StockTorch:
    """y = conv1d(pad(x), W, stride=M) transposed: W[c][u] = h32[c M + half - (u - left) L]"""

    def __init__(self, h, L, M, dev):
        h32 = np.asarray(h, dtype=np.float64).astype(np.float32)
        half = (len(h32) - 1) // 2
        self.L, self.M, self.left = L, M, -(-half // L)
        self.width = self.left + ((L - 1) * M + half) // L + 1
        idx = (np.arange(L)[:, None] * M + half) - (np.arange(self.width)[None, :] - self.left) * L
        ok = (idx >= 0) & (idx < len(h32))
        self.weight = torch.from_numpy(np.where(ok, h32[np.clip(idx, 0, len(h32) - 1)], np.float32(0))[:, None, :].copy()).to(dev)

    def __call__(self, x):
        B, N = x.shape
        No = -(-N * self.L // self.M)
        frames = -(-No // self.L)
        right = max(0, (frames - 1) * self.M + self.width - self.left - N)
        y = F.conv1d(F.pad(x, (self.left, right))[:, None, :], self.weight, stride=self.M)
        return y.transpose(1, 2).reshape(B, -1)[:, :No]


def case(a, b, quality, sigs, dev, steps, warmup, with_stock, with_scipy):
    L, M, h = RS.resample_filter(a, b, quality)
    lens = [len(s) for s in sigs]
    B, N = len(sigs), max(lens)
    host = np.zeros((B, N), np.float32)
    for i, s in enumerate(sigs):
        host[i, :lens[i]] = s
    x = torch.from_numpy(host).to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    ms, (out, out_lens) = timed(lambda: RS.resample(x, lens_d, a, b, quality), steps, warmup)
    olens = out_lens.tolist()
    taps = -(-len(h) // L)
    n_in, n_out = sum(lens), sum(olens)
    res = {"from": a, "to": b, "quality": quality, "L": L, "M": M, "taps": len(h), "taps_per_output": taps, "padded_shape": [B, N],
           "out_shape": list(out.shape), "ms_per_call": round(ms, 4), "input_samples_per_s": round(n_in / (ms * 1e-3), 1),
           "audio_s_per_s": round(n_in / a / (ms * 1e-3), 1),
           "bytes_per_s": round(4.0 * (n_in + n_out) / (ms * 1e-3), 1), "fraction_of_8_TB_s": round(4.0 * (n_in + n_out) / (ms * 1e-3) / HBM_BYTES_PER_S, 5),
           "fma_per_s": round(n_out * taps / (ms * 1e-3), 1), "fraction_of_fp32_vector_peak": round(n_out * taps / (ms * 1e-3) / FP32_VECTOR_FMA_PER_S, 5)}
    if with_stock:
        stock = StockTorch(h, L, M, dev)
        sms, y = timed(lambda: stock(x), steps, warmup)
        diff = 0.0
        for i, n in enumerate(olens):                           # the stock form filters the padded row: compare full-length rows only where equal
            if lens[i] == N:
                diff = max(diff, float((y[i, :n] - out[i, :n]).abs().max()))
        res.update({"stock_torch_ms_per_call": round(sms, 4), "stock_torch_kernel_shape": list(stock.weight.shape),
                    "speedup_vs_stock_torch": round(sms / ms, 3), "max_abs_diff_vs_stock_torch_longest_row": diff})
    if with_scipy:
        try:
            from scipy.signal import resample_poly
            t0 = time.perf_counter()
            ys = resample_poly(sigs[0].astype(np.float64), L, M, window=h / L, padtype="constant")
            res["scipy_host_ms_one_utterance"] = round((time.perf_counter() - t0) * 1e3, 3)
            res["scipy_host_utterance_samples"] = lens[0]
            res["max_abs_diff_vs_scipy"] = float(np.abs(out[0, :olens[0]].cpu().numpy() - ys).max())
        except ImportError:
            res["scipy_host_ms_one_utterance"] = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = [min(int(v), 1024) for v in make_batch(seed=1234)["mel_lens"]]
    len22 = [256 * f for f in frames]
    sig48 = [speechlike(n * 320 // 147, 48000, 500 + i) for i, n in enumerate(len22)]       # ceil(len48 147 / 320) == len22
    sig22 = [speechlike(n, 22050, 500 + i) for i, n in enumerate(len22)]
    cases = [case(48000, 22050, "kaiser_best", sig48, dev, a.steps, a.warmup, True, True),
             case(48000, 22050, "kaiser_fast", sig48, dev, a.steps, a.warmup, True, False),
             case(22050, 48000, "kaiser_best", sig22, dev, a.steps, a.warmup, True, False)]
    best = cases[0]
    res = {"tool": "tools/bench_resample.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "batch": {"utterances": len(frames), "frames": frames, "audio_s": round(sum(len22) / 22050.0, 2)},
           "cases": cases,
           "bar": "native not slower than the stock-torch formulation of the same run at kaiser_best, 48000 -> 22050, canonical batch",
           "bar_ratio": best["speedup_vs_stock_torch"], "bar_met": bool(best["speedup_vs_stock_torch"] >= 1.0),
           "note": "parity with librosa / resampy is UNPINNED (neither is installed): the kernel is pinned against a float64 restatement of "
                   "the windowed-sinc definition, which equals scipy.signal.resample_poly with the same window",
           "steps": a.steps, "warmup": a.warmup}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
