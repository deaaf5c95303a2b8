"""Loudness metering and normalisation on the device (csrc/loudness.hip through ctts_amd.loudness) against a stock-torch formulation of
the same chain on the same device and the float64 restatement on the host, timed in the same run.  Prints ONE JSON line.

Batch: the canonical 16 speech-like utterances of tools/bench_resample.py (synthetic.make_batch()'s mel lengths capped at 1024; 256
samples per frame at 22.05 kHz, 139 s of audio), synthesised at 22050 Hz and at 48000 Hz.  Timing: warm-up, then the median over HIP
events around back-to-back calls (tools/bench_pitch_features.timed).  Per rate: `integrated_loudness` and `normalize_loudness` per call
(these include the host's share: lengths and block counts go to the device with every call), the three stages on their own
(`kernels.kweight_energy`: zero-state pass + state scan + energy pass; `kernels.loudness_gate`; `kernels.apply_gain`), achieved
bytes / s against 6.3 TB/s counting 4 bytes per sample for the measurement (each sample is fetched twice, by the zero-state pass and by
the energy pass; the second fetch is counted as well in `bytes_per_s_both_passes`) and 8 bytes per sample for the gain.
Stock torch: K-weighting as an rFFT-domain product - the two biquads' frequency response, evaluated in float64 on the grid of the
zero-padded batch (padded by at least 16384 samples, up to a length 2^a 3^b 5^c, so that the recursion's tail does not wrap), times `torch.fft.rfft` of the batch in fp32 -
then `irfft`, squares masked to each utterance's length, hop sums by a reshape (both rates have a whole number of samples per 0.1 s),
block sums by `unfold(1, 4, 1)`, and the two gates with masks.  Its loudness is compared with float64 like the kernel's.
Host: tests/loudness_restate.py (scipy.signal.lfilter in float64) on the first utterance.
No speed bar is set: this chain had not been measured here before.  Parity with pyloudnorm is UNPINNED (it is not installed).

    python tools/bench_loudness.py [--steps 20] [--warmup 3] [--out profiles/loudness_bench.json]"""
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
from ctts_amd import kernels as K, loudness as LD  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402
from bench_pitch_features import timed  # noqa: E402
from bench_resample import speechlike  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
FFT_TAIL = 16384


def _smooth(n):
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


class StockTorch:
    """the same measurement from stock torch ops (module docstring)"""

    def __init__(self, rate, N, lens, dev):
        from scipy.signal import freqz
        self.rate, self.N, self.hop = rate, N, rate // 10
        assert self.hop * 10 == rate
        self.nfft = (N + FFT_TAIL + 1) // 2 * 2
        while not _smooth(self.nfft):                    # a length the FFT library has radices for: 2^a 3^b 5^c
            self.nfft += 2
        w = np.arange(self.nfft // 2 + 1) * (2 * np.pi / self.nfft)
        H = np.ones(len(w), dtype=np.complex128)
        for b, a in LD.kweighting(rate):
            H = H * freqz(b, a, worN=w)[1]
        self.H = torch.from_numpy(H.astype(np.complex64)).to(dev)
        self.lens = torch.tensor(lens, device=dev)
        self.nb = torch.tensor([LD.n_blocks(n, rate) for n in lens], device=dev)
        self.J = int(self.nb.max())
        self.mask = (torch.arange(N, device=dev)[None, :] < self.lens[:, None])
        self.live = (torch.arange(self.J, device=dev)[None, :] < self.nb[:, None])

    def __call__(self, x):
        y = torch.fft.irfft(torch.fft.rfft(x, n=self.nfft) * self.H, n=self.nfft)[:, :self.N]
        e = torch.where(self.mask, y * y, torch.zeros((), device=x.device))
        need = (self.J + 3) * self.hop
        e = torch.nn.functional.pad(e, (0, max(0, need - self.N)))[:, :need]
        z = e.reshape(x.shape[0], self.J + 3, self.hop).sum(2).unfold(1, 4, 1).sum(2) / (0.4 * self.rate)
        l = -0.691 + 10 * torch.log10(z)
        first = self.live & (l >= -70.0)
        gr = -0.691 + 10 * torch.log10((z * first).sum(1) / first.sum(1)) - 10.0
        second = self.live & (l > gr[:, None]) & (l > -70.0)
        return -0.691 + 10 * torch.log10((z * second).sum(1) / second.sum(1))


def case(rate, sigs, dev, steps, warmup):
    import loudness_restate as R
    lens = [len(s) for s in sigs]
    B, N = len(sigs), max(lens)
    host = np.zeros((B, N), np.float32)
    for i, s in enumerate(sigs):
        host[i, :lens[i]] = s
    x = torch.from_numpy(host).to(dev)
    n_in = sum(lens)
    ms_int, (loud, valid) = timed(lambda: LD.integrated_loudness(x, lens, rate), steps, warmup)
    ms_norm, (out, _, gain, _) = timed(lambda: LD.normalize_loudness(x, lens, rate), steps, warmup)
    # the stages on their own, on tensors prepared once
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    nb_d = torch.tensor([LD.n_blocks(n, rate) for n in lens], dtype=torch.int32, device=dev)
    edges, chunk_seg, blocks = LD._tables(rate, "momentary", N, dev)
    coef = LD._coef(rate, dev)
    ms_kw, (hop_sums, peak) = timed(lambda: K.kweight_energy(x, lens_d, coef, edges, chunk_seg), steps, warmup)
    ms_gate, _ = timed(lambda: K.loudness_gate(hop_sums, lens_d, nb_d, edges, chunk_seg, blocks, peak, N, 0.4 * rate), steps, warmup)
    ms_gain, _ = timed(lambda: K.apply_gain(x, lens_d, gain), steps, warmup)
    stock = StockTorch(rate, N, lens, dev)
    ms_stock, l_stock = timed(lambda: stock(x), steps, warmup)
    t0 = time.perf_counter()
    L0, _ = R.integrated_loudness(sigs[0].astype(np.float64), rate)
    host_ms = (time.perf_counter() - t0) * 1e3
    L64 = np.array([R.integrated_loudness(s.astype(np.float64), rate)[0] for s in sigs])
    L32 = np.array([R.integrated_loudness(s, rate, dtype=np.float32)[0] for s in sigs])
    sec = ms_kw * 1e-3
    return {"rate": rate, "padded_shape": [B, N], "samples": n_in, "audio_s": round(n_in / rate, 2), "chunk": K.loudness_chunk(),
            "integrated_loudness_ms_per_call": round(ms_int, 4), "normalize_loudness_ms_per_call": round(ms_norm, 4),
            "kweight_energy_ms": round(ms_kw, 4), "loudness_gate_ms": round(ms_gate, 4), "apply_gain_ms": round(ms_gain, 4),
            "audio_s_per_s_integrated": round(n_in / rate / (ms_int * 1e-3), 1),
            "kweight_energy_samples_per_s": round(n_in / sec, 1),
            "kweight_energy_bytes_per_s": round(4.0 * n_in / sec, 1), "kweight_energy_fraction_of_6_3_TB_s": round(4.0 * n_in / sec / HBM_BYTES_PER_S, 5),
            "bytes_per_s_both_passes": round(8.0 * n_in / sec, 1),
            "apply_gain_bytes_per_s": round(8.0 * B * N / (ms_gain * 1e-3), 1),
            "apply_gain_fraction_of_6_3_TB_s": round(8.0 * B * N / (ms_gain * 1e-3) / HBM_BYTES_PER_S, 5),
            "stock_torch_ms_per_call": round(ms_stock, 4), "stock_torch_fft_length": stock.nfft,
            "speedup_vs_stock_torch_stages": round(ms_stock / (ms_kw + ms_gate), 3),
            "speedup_vs_stock_torch_call": round(ms_stock / ms_int, 3),
            "max_err_LU_kernel_vs_float64": float(np.max(np.abs(loud.cpu().numpy() - L64))),
            "max_err_LU_stock_torch_vs_float64": float(np.max(np.abs(l_stock.double().cpu().numpy() - L64))),
            "max_err_LU_float32_lfilter_vs_float64": float(np.max(np.abs(L32 - L64))),
            "loudness_first_utterance": float(L0), "valid": int(valid.sum()),
            "restatement_host_ms_one_utterance": round(host_ms, 3), "restatement_utterance_samples": lens[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = [min(int(v), 1024) for v in make_batch(seed=1234)["mel_lens"]]
    len22 = [256 * f for f in frames]
    sig22 = [speechlike(n, 22050, 500 + i) for i, n in enumerate(len22)]
    sig48 = [speechlike(n * 320 // 147, 48000, 500 + i) for i, n in enumerate(len22)]
    cases = [case(22050, sig22, dev, a.steps, a.warmup), case(48000, sig48, dev, a.steps, a.warmup)]
    res = {"tool": "tools/bench_loudness.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "batch": {"utterances": len(frames), "frames": frames, "audio_s": round(sum(len22) / 22050.0, 2)},
           "cases": cases,
           "stock_torch": "rfft of the zero-padded batch times the biquads' response, irfft, masked squares, hop sums by reshape, blocks by "
                          "unfold, gates by masks (fp32)",
           "note": "parity with pyloudnorm is UNPINNED (it is not installed): the kernels are pinned against the float64 restatement of "
                   "BS.1770-4 in tests/loudness_restate.py; no speed bar was set in advance",
           "steps": a.steps, "warmup": a.warmup}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
