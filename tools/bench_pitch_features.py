"""Pitch targets on the device: the native tracker and target chain (csrc/pitchtrack.hip through ctts_amd.pitch_features) against a
stock-torch device implementation of the SAME two algorithms in the same process (torch.fft, batched: frames by unfold, rfft / irfft of
2048 points, masked argmax; the chain with cummax scans and one fft / ifft per utterance at its own power of two, the utterance
lengths known on the host).  Prints ONE JSON line.

Batch: the canonical 16 utterances (synthetic.make_batch()'s mel lengths capped at 1024: 11 992 frames, 256 (F - 1) samples each) of
speech-like harmonic audio - a gliding fundamental with six harmonics under a syllable envelope, noise bursts between the voiced
stretches.  Reported: median time per call over HIP events around 10 back-to-back calls (tracker = peak launch + tracker launch; chain = f0_targets + norm_interp_f0), the
tracker kernel's own device time from a torch.profiler trace, frames per second, the stock times and the ratios, and how far the two
implementations are apart (they are float32 restatements of one algorithm: voicing decisions may differ on frames at a threshold).

    python tools/bench_pitch_features.py [--steps 20] [--warmup 3] [--out profiles/pitch_features_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctts_amd  # noqa: E402,F401
from ctts_amd import kernels as K, pitch_features as PF  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402

SR, HOP, FRAME, NFFT = 22050, 256, 1024, 2048
F0_MIN, F0_MAX, VTHR, STHR = 80.0, 750.0, 0.6, 0.03


def timed(fn, steps, warmup, inner=10):
    """median over `steps` windows of `inner` back-to-back calls each (HIP events), in ms per call"""
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return statistics.median(ts), out


def kernel_us(fn, name):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    tot, cnt = 0.0, 0
    for e in prof.key_averages():
        if name in e.key:
            tot += getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
            cnt += e.count
    return tot / cnt if cnt else None


def speechlike_wave(n, seed):
    """gliding fundamental (90 - 260 Hz) + 5 harmonics, syllable envelope, noise in the unvoiced stretches"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    f = 150.0 + 60.0 * np.sin(2 * np.pi * (0.7 + 0.3 * rng.random()) * t + rng.random() * 6) + 30.0 * np.sin(2 * np.pi * 2.3 * t)
    ph = 2 * np.pi * np.cumsum(f) / SR
    x = sum(np.sin(k * ph) / k for k in range(1, 7))
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t + rng.random() * 6)
    voiced = np.sin(2 * np.pi * 1.3 * t + rng.random() * 6) > -0.5
    y = np.where(voiced, 0.3 * x * env, 0.02 * rng.standard_normal(n))
    return np.clip(y, -1, 1).astype(np.float32)


class StockPitch:
    """the two algorithms of include/ctts.h on stock torch device ops"""

    def __init__(self, dev):
        n = torch.arange(FRAME, dtype=torch.float64)
        w = 0.5 - 0.5 * torch.cos(2 * math.pi * n / FRAME)
        rw = torch.stack([(w[:FRAME - t] * w[t:]).sum() for t in range(512)])
        self.win = w.float().to(dev)
        self.rwn = (rw / rw[0]).float().to(dev)
        self.lo, self.hi = int(math.floor(SR / F0_MAX)), int(math.ceil(SR / F0_MIN))
        self.dev = dev

    def track(self, wav, lens):
        B, N = wav.shape
        F = 1 + N // HOP
        idx = torch.arange(N, device=self.dev)[None, :]
        x = torch.where(idx < lens[:, None], wav, torch.zeros_like(wav))
        peak = x.abs().amax(1)
        xp = torch.nn.functional.pad(x, (FRAME // 2, FRAME // 2 + HOP))
        fr = xp.unfold(1, FRAME, HOP)[:, :F]
        amax = fr.abs().amax(-1)
        xw = (fr - fr.mean(-1, keepdim=True)) * self.win
        X = torch.fft.rfft(xw, NFFT)
        r = torch.fft.irfft(X.real * X.real + X.imag * X.imag, NFFT)[..., :512]
        r0 = r[..., :1]
        ok = (r0 > 0) & torch.isfinite(r0)
        rn = torch.where(ok, r / torch.where(ok, r0, torch.ones_like(r0)), torch.zeros_like(r)) / self.rwn
        a, b, c = rn[..., self.lo - 1:self.hi], rn[..., self.lo:self.hi + 1], rn[..., self.lo + 1:self.hi + 2]
        cand = (b > a) & (b >= c)
        den = torch.where(cand, (a - b) + (c - b), torch.full_like(a, -1.0))
        dl = 0.5 * (a - c) / den
        lag = torch.arange(self.lo, self.hi + 1, device=self.dev, dtype=torch.float32) + dl
        h = b - 0.25 * (a - c) * dl
        cost = torch.where(cand, h - 0.01 * torch.log2(F0_MIN * lag / SR), torch.full_like(h, -float("inf")))
        w = cost.argmax(-1, keepdim=True)
        any_c = cand.any(-1)
        hw, lw = h.gather(-1, w)[..., 0], lag.gather(-1, w)[..., 0]
        live = torch.arange(F, device=self.dev)[None, :] < (1 + torch.div(lens, HOP, rounding_mode="floor"))[:, None]
        st = torch.where(any_c & live, hw, torch.zeros_like(hw))
        voiced = any_c & live & (hw >= VTHR) & (amax >= STHR * peak[:, None])
        return torch.where(voiced, SR / lw, torch.zeros_like(lw)), st

    def chain(self, f0, frames_host):
        """per utterance (host lengths): continuous log-F0 by cummax scans, mean / std, CWT at the utterance's own power of two"""
        B, F = f0.shape
        uv = torch.zeros_like(f0)
        cont = torch.zeros_like(f0)
        cwt = torch.zeros(B, F, 10, device=self.dev)
        ms = torch.zeros(B, 2, device=self.dev)
        for b, n in enumerate(frames_host):
            x = f0[b, :n]
            t = torch.arange(n, device=self.dev)
            nz = x != 0
            prev = torch.cummax(torch.where(nz, t, torch.full_like(t, -1)), 0)[0]
            nxt = torch.flip(torch.cummin(torch.flip(torch.where(nz, t, torch.full_like(t, n)), [0]), 0)[0], [0])
            p, q = prev.clamp(min=0), nxt.clamp(max=n - 1)
            yp, yq = x[p], x[q]
            mid = yp + (yq - yp) / (q - p).clamp(min=1) * (t - p)
            y = torch.where(prev < 0, yq, torch.where(nxt >= n, yp, torch.where(nz, x, mid)))
            lf = torch.log(y)
            mean, std = lf.mean(), lf.std(unbiased=False)
            M = 1 << max(n - 1, 0).bit_length()
            X = torch.fft.fft((lf - mean) / std, M)
            w = 2 * math.pi * torch.fft.fftfreq(M, 0.005, device=self.dev)
            s = (0.01 * 2.0 ** torch.arange(10, device=self.dev))[:, None]
            fw = s * w[None, :]
            psi = torch.sqrt(s * (2 * math.pi / 0.005)) * fw * fw * torch.exp(-0.5 * fw * fw) / math.sqrt(math.gamma(2.5))
            cwt[b, :n] = torch.fft.ifft(X[None, :] * psi, dim=-1)[:, :n].real.t()
            uv[b, :n], cont[b, :n], ms[b, 0], ms[b, 1] = (~nz).float(), lf, mean, std
        return uv, cont, ms, cwt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_features_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = [min(int(v), 1024) for v in make_batch(seed=1234)["mel_lens"]]
    lens = [HOP * (F - 1) for F in frames]
    B, N = len(lens), max(lens)
    wav_h = np.zeros((B, N), np.float32)
    for b, n in enumerate(lens):
        wav_h[b, :n] = speechlike_wave(n, 300 + b)
    wav = torch.from_numpy(wav_h).to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    frames_d = torch.tensor(frames, dtype=torch.int32, device=dev)
    PF.prepare(dev)
    stock = StockPitch(dev)

    trk_ms, (f0, st) = timed(lambda: PF.track_pitch(wav, lens_d), a.steps, a.warmup)
    trk_kernel = kernel_us(lambda: PF.track_pitch(wav, lens_d), "pitch_track_kernel")
    chain_ms, tg = timed(lambda: (PF.f0_targets(f0, frames_d), K.norm_interp_f0(f0, frames_d)), a.steps, a.warmup)
    chain_kernel = kernel_us(lambda: PF.f0_targets(f0, frames_d), "f0_targets_kernel")
    s_trk_ms, (sf0, sst) = timed(lambda: stock.track(wav, lens_d), a.steps, a.warmup)
    s_chain_ms, (suv, scont, sms, scwt) = timed(lambda: stock.chain(f0, frames), a.steps, a.warmup)
    tg = tg[0]
    n_frames = sum(frames)
    both = (f0 > 0) & (sf0 > 0)
    res = {
        "tool": "tools/bench_pitch_features.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
        "batch": {"utterances": B, "frames": n_frames, "audio_s": round(sum(lens) / SR, 2), "voiced_frames": int((f0 > 0).sum())},
        "tracker_us": round(trk_ms * 1e3, 1), "tracker_kernel_us": None if trk_kernel is None else round(trk_kernel, 1),
        "tracker_frames_per_s": round(n_frames / (trk_ms * 1e-3)),
        "chain_us": round(chain_ms * 1e3, 1), "chain_kernel_us": None if chain_kernel is None else round(chain_kernel, 1),
        "stock_tracker_us": round(s_trk_ms * 1e3, 1), "stock_chain_us": round(s_chain_ms * 1e3, 1),
        "tracker_speedup_vs_stock": round(s_trk_ms / trk_ms, 2), "chain_speedup_vs_stock": round(s_chain_ms / chain_ms, 2),
        "native_vs_stock": {
            "voicing_mismatch_frames": int(((f0 > 0) != (sf0 > 0)).sum()),
            "f0_max_rel": float(((f0 - sf0).abs() / sf0.clamp(min=1))[both].max()) if both.any() else None,
            "cwt_max_abs": float((tg["cwt_spec"] - scwt).abs().max()), "valid": int(tg["valid"].sum()),
        },
        "steps": a.steps, "warmup": a.warmup,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
