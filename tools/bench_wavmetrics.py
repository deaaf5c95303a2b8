"""Waveform metrics on the device (csrc/wavmetrics.hip through ctts_amd.metrics) against a stock-torch formulation of the same chain on
the same device and the float64 restatement on the host, timed in the same run.  Prints ONE JSON line.

Batch: the canonical 16 speech-like utterances of tools/bench_resample.py (synthetic.make_batch()'s mel lengths capped at 1024; 256
samples per frame at 22.05 kHz, 139 s of audio) as the recordings, each plus white noise at 10 dB as the synthesised side.  Timing:
warm-up, then the median over HIP events around back-to-back calls (tools/bench_pitch_features.timed).  Native: `waveform_metrics` per
call at 22050 Hz (the resample of both signals to 10 kHz included), then the stages on their own on tensors prepared once:
`kernels.stoi` on the resampled batch, `kernels.si_sdr`, the three `kernels.mr_stft` resolutions.
Stock torch (fp32, the way one would port pystoi and the Parallel-WaveGAN loss): per utterance, frames by `unfold`, the energy mask,
boolean indexing of the kept frames (a host synchronisation per utterance - the formulation has no way round it), overlap-add by
`index_add_`, frames again, `torch.fft.rfft`, the 15 bands as a matmul with a 0 / 1 matrix, segments by `unfold`, STOI and ESTOI from
tensor ops; SI-SDR from dot products; the STFT distances from `torch.stft(center=False)` on the padded batch with frames beyond each
length masked.  It starts from the same resampled audio, so the resampler is not part of its time.
Host: tests/wavmetrics_restate.py in float64 on the first utterance (timed) and on all (errors).
No speed bar is set: this chain had not been measured here before.  Parity with pystoi is UNPINNED (it is not installed).

    python tools/bench_wavmetrics.py [--steps 20] [--warmup 3] [--out profiles/wavmetrics_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import kernels as K, metrics as M, resample as RS  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402
from bench_pitch_features import timed  # noqa: E402
from bench_resample import speechlike  # noqa: E402

RATE = 22050


class StockTorch:
    """the same numbers from stock torch ops in fp32 (module docstring)"""

    def __init__(self, dev):
        import wavmetrics_restate as R
        self.w = torch.from_numpy(R.window().astype(np.float32)).to(dev)
        band = np.zeros((257, 15), dtype=np.float32)
        for j, (lo, hi) in enumerate(R.band_edges()):
            band[lo:hi, j] = 1.0
        self.band = torch.from_numpy(band).to(dev)
        self.clip = 1.0 + 10.0 ** (15.0 / 20.0)
        self.eps = float(np.finfo(np.float32).eps)
        self.mrw = {win: torch.from_numpy(R.mr_window(win).astype(np.float32)).to(dev) for _, _, win in M.MR_STFT_DEFAULT}

    def _bands(self, v, keep):
        fr = (v.unfold(0, 256, 128) * self.w)[keep]
        k = fr.shape[0]
        out = torch.zeros(128 * (k - 1) + 256, device=v.device)
        pos = (128 * torch.arange(k, device=v.device)[:, None] + torch.arange(256, device=v.device)[None, :]).reshape(-1)
        out.index_add_(0, pos, fr.reshape(-1))
        spec = torch.fft.rfft(out.unfold(0, 256, 128) * self.w, n=512)
        return torch.sqrt((spec.real ** 2 + spec.imag ** 2) @ self.band).t().unfold(1, 30, 1).permute(1, 0, 2)      # [S, 15, 30]

    def stoi(self, x, y, lens):
        res = []
        for b, n in enumerate(lens):
            xb, yb = x[b, :n], y[b, :n]
            e = 20 * torch.log10(torch.linalg.norm(xb.unfold(0, 256, 128) * self.w, dim=1) + self.eps)
            keep = e > e.max() - 40.0
            X, Y = self._bands(xb, keep), self._bands(yb, keep)
            alpha = torch.linalg.norm(X, dim=2, keepdim=True) / (torch.linalg.norm(Y, dim=2, keepdim=True) + self.eps)
            Yp = torch.minimum(alpha * Y, X * self.clip)
            Xc, Yc = X - X.mean(2, keepdim=True), Yp - Yp.mean(2, keepdim=True)
            d = ((Xc / (torch.linalg.norm(Xc, dim=2, keepdim=True) + self.eps)) * (Yc / (torch.linalg.norm(Yc, dim=2, keepdim=True) + self.eps))).sum()
            d = d / (15 * X.shape[0])

            def rowcol(a):
                a = a - a.mean(2, keepdim=True)
                a = a / (torch.linalg.norm(a, dim=2, keepdim=True) + self.eps)
                a = a - a.mean(1, keepdim=True)
                return a / (torch.linalg.norm(a, dim=1, keepdim=True) + self.eps)
            res.append(torch.stack([d, (rowcol(X) * rowcol(Y)).sum() / (30 * X.shape[0])]))
        return torch.stack(res)

    def si_sdr(self, x, y, mask, n):
        xc = torch.where(mask, x - (x * mask).sum(1, keepdim=True) / n, torch.zeros((), device=x.device))
        yc = torch.where(mask, y - (y * mask).sum(1, keepdim=True) / n, torch.zeros((), device=x.device))
        t = ((yc * xc).sum(1, keepdim=True) / (xc * xc).sum(1, keepdim=True)) * xc
        return 10 * torch.log10((t * t).sum(1) / ((yc - t) ** 2).sum(1))

    def mr(self, x, y, lens_t):
        out = []
        for n_fft, hop, win in M.MR_STFT_DEFAULT:
            w = torch.nn.functional.pad(self.mrw[win], (0, n_fft - win))
            nf = torch.div(lens_t - win, hop, rounding_mode="floor") + 1
            mx, my = (torch.sqrt(torch.clamp(torch.stft(v, n_fft, hop, n_fft, w, center=False, return_complex=True).abs() ** 2, min=1e-7))
                      for v in (x, y))
            live = (torch.arange(mx.shape[2], device=x.device)[None, :] < nf[:, None])[:, None, :]
            zero = torch.zeros((), device=x.device)
            sc = torch.sqrt(torch.where(live, (mx - my) ** 2, zero).sum((1, 2))) / torch.sqrt(torch.where(live, mx * mx, zero).sum((1, 2)))
            lm = torch.where(live, (mx.log() - my.log()).abs(), zero).sum((1, 2)) / (nf * mx.shape[1])
            lsd = torch.where(live[:, 0], torch.sqrt(((20 * mx.log10() - 20 * my.log10()) ** 2).mean(1)), zero).sum(1) / nf
            out.append(torch.stack([sc, lm, lsd], dim=1))
        return torch.stack(out, dim=1)                                       # [B, R, 3]


def main():
    import wavmetrics_restate as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavmetrics_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = [min(int(v), 1024) for v in make_batch(seed=1234)["mel_lens"]]
    lens = [256 * f for f in frames]
    refs = [speechlike(n, RATE, 500 + i) for i, n in enumerate(lens)]
    rng = np.random.default_rng(77)
    syns = []
    for r in refs:
        n = rng.standard_normal(len(r))
        syns.append((r + n * np.sqrt(np.mean(r.astype(np.float64) ** 2) / np.mean(n ** 2)) * 10.0 ** (-10.0 / 20.0)).astype(np.float32))
    B, N = len(refs), max(lens)
    host = np.zeros((2, B, N), np.float32)
    for i in range(B):
        host[0, i, :lens[i]], host[1, i, :lens[i]] = refs[i], syns[i]
    x, y = torch.from_numpy(host[0]).to(dev), torch.from_numpy(host[1]).to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    ms_call, got = timed(lambda: M.waveform_metrics(x, y, lens, RATE), a.steps, a.warmup)
    ms_res, (x10, lens10_d) = timed(lambda: RS.resample(x, lens_d, RATE, 10000), a.steps, a.warmup)
    y10, _ = RS.resample(y, lens_d, RATE, 10000)
    lens10 = lens10_d.tolist()
    win = torch.from_numpy(M.stoi_window()).to(dev)
    ms_stoi, _ = timed(lambda: K.stoi(x10, y10, lens10_d, win), a.steps, a.warmup)
    ms_sd, _ = timed(lambda: K.si_sdr(x, y, lens_d), a.steps, a.warmup)
    mrw = [torch.from_numpy(M.mr_stft_window(w)).to(dev) for _, _, w in M.MR_STFT_DEFAULT]
    ms_mr, _ = timed(lambda: [K.mr_stft(x, y, lens_d, mrw[r], n, h) for r, (n, h, _) in enumerate(M.MR_STFT_DEFAULT)], a.steps, a.warmup)
    stock = StockTorch(dev)
    mask = torch.arange(N, device=dev)[None, :] < lens_d[:, None]
    nf = lens_d[:, None].float()
    ms_s_stoi, s_stoi = timed(lambda: stock.stoi(x10, y10, lens10), a.steps, a.warmup)
    ms_s_sd, s_sd = timed(lambda: stock.si_sdr(x, y, mask, nf), a.steps, a.warmup)
    ms_s_mr, s_mr = timed(lambda: stock.mr(x, y, lens_d), a.steps, a.warmup)
    # float64 on the host: STOI / ESTOI on the device's resampled audio, the rest on the 22.05 kHz signals
    x10h, y10h = x10.cpu().numpy(), y10.cpu().numpy()
    t0 = time.perf_counter()
    first = (R.stoi(x10h[0, :lens10[0]], y10h[0, :lens10[0]]), R.si_sdr(refs[0], syns[0]), R.mr_stft_distance(refs[0], syns[0]))
    host_ms = (time.perf_counter() - t0) * 1e3
    w_stoi = [first[0]] + [R.stoi(x10h[i, :lens10[i]], y10h[i, :lens10[i]]) for i in range(1, B)]
    w_sd = np.array([first[1]] + [R.si_sdr(refs[i], syns[i]) for i in range(1, B)])
    w_mr = [first[2]] + [R.mr_stft_distance(refs[i], syns[i]) for i in range(1, B)]
    want = {"stoi": np.array([v["stoi"] for v in w_stoi]), "estoi": np.array([v["estoi"] for v in w_stoi]), "si_sdr": w_sd,
            "sc": np.stack([v["sc"] for v in w_mr]), "log_mag": np.stack([v["log_mag"] for v in w_mr]),
            "lsd_db": np.stack([v["lsd_db"] for v in w_mr])}
    s_stoi, s_mr = s_stoi.double().cpu().numpy(), s_mr.double().cpu().numpy()
    stock_v = {"stoi": s_stoi[:, 0], "estoi": s_stoi[:, 1], "si_sdr": s_sd.double().cpu().numpy(), "sc": s_mr[:, :, 0], "log_mag": s_mr[:, :, 1],
               "lsd_db": s_mr[:, :, 2]}
    assert [v["segments"] for v in w_stoi] == got["segments"].tolist() and [v["kept"] for v in w_stoi] == got["kept"].tolist()
    native_stages, stock_total = ms_stoi + ms_sd + ms_mr, ms_s_stoi + ms_s_sd + ms_s_mr
    summary = M.summarize_waveform(got)
    res = {"tool": "tools/bench_wavmetrics.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "batch": {"utterances": B, "frames": frames, "audio_s": round(sum(lens) / float(RATE), 2), "rate": RATE, "snr_db": 10.0,
                     "stoi_frames": int(got["frames"].sum()), "stoi_kept": int(got["kept"].sum()), "stoi_segments": int(got["segments"].sum()),
                     "mr_frames": got["mr_frames"].sum(0).tolist()},
           "waveform_metrics_ms_per_call": round(ms_call, 4), "audio_s_per_s": round(sum(lens) / float(RATE) / (ms_call * 1e-3), 1),
           "resample_one_signal_ms": round(ms_res, 4), "stoi_estoi_ms": round(ms_stoi, 4), "si_sdr_ms": round(ms_sd, 4),
           "mr_stft_ms": round(ms_mr, 4), "native_stages_ms": round(native_stages, 4),
           "stock_torch_stoi_estoi_ms": round(ms_s_stoi, 4), "stock_torch_si_sdr_ms": round(ms_s_sd, 4), "stock_torch_mr_stft_ms": round(ms_s_mr, 4),
           "stock_torch_stages_ms": round(stock_total, 4), "speedup_vs_stock_torch_stages": round(stock_total / native_stages, 3),
           "speedup_stoi_estoi": round(ms_s_stoi / ms_stoi, 3), "speedup_si_sdr": round(ms_s_sd / ms_sd, 3),
           "speedup_mr_stft": round(ms_s_mr / ms_mr, 3),
           "max_err_kernel_vs_float64": {k: float(np.max(np.abs(got[k].cpu().numpy() - want[k]))) for k in want},
           "max_err_stock_torch_fp32_vs_float64": {k: float(np.max(np.abs(stock_v[k] - want[k]))) for k in want},
           "corpus_means": {k: summary[k]["mean"] for k in ("stoi", "estoi", "si_sdr", "sc", "log_mag", "lsd_db")},
           "restatement_host_ms_one_utterance": round(host_ms, 3), "restatement_utterance_samples": lens[0],
           "stock_torch": "per utterance: unfold, energy mask, boolean indexing (host sync), index_add_ overlap-add, rfft, band matmul, "
                          "unfold segments; dot-product SI-SDR; torch.stft(center=False) with masked frames (fp32)",
           "note": "parity with pystoi is UNPINNED (it is not installed; its resampler differs): the kernels are pinned against the float64 "
                   "restatement in tests/wavmetrics_restate.py; no speed bar was set in advance",
           "steps": a.steps, "warmup": a.warmup}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
