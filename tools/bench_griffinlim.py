"""Griffin-Lim, 60 iterations: the native path (csrc/griffinlim.hip through ctts_amd.audio.griffin_lim, ragged batch in one launch per
iteration) against stock torch on the same GPU in the same process - the reference algorithm (audio/stft.py:59-127,
audio/audio_processing.py:66-82) restated with conv1d / conv_transpose1d on the same [1026 x 1024] windowed bases (as the
equivalent GEMMs with unfold / fold, tests/griffinlim_restate.py StockSTFT), one utterance
per call as the reference runs it (16 separate 60-iteration loops: much of that time is kernel-launch overhead), and as one zero-padded
batch (the fairer algorithmic comparison; its frames near the padded end are not the per-utterance result).  Prints ONE JSON line.

Shapes: B = 16 utterances of the canonical mel lengths (synthetic.make_batch()'s mel_lens, capped at 1024 frames) and one 870-frame
utterance.  Per shape: median ms over HIP events, audio-seconds per second, the device time of one gl_iter_kernel launch from a
torch.profiler kernel trace (iter_kernel_us; iter_loop_us is the event time of 60 back-to-back launches / 60, launch gaps included),
its algorithmic HBM bytes (Y_in 4 KB + target magnitude 2052 B + Y_out 4 KB per frame) over the kernel time against 8 TB/s, and the
relative L2 distance between native and stock outputs.

    python tools/bench_griffinlim.py [--steps 10] [--warmup 2] [--out profiles/griffinlim_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctts_amd  # noqa: E402,F401
from ctts_amd import audio, kernels as K  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
from griffinlim_restate import StockSTFT  # noqa: E402

NFFT, HOP, SR, ITERS, PEAK_TBS = 1024, 256, 22050, 60, 8.0
BYTES_PER_FRAME = 4 * (NFFT + 513 + NFFT)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), out


def kernel_us(fn, name):
    """mean device time (us) of the kernels whose name contains `name`, from a torch.profiler trace of one call of fn"""
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


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stft = audio.STFT(NFFT, HOP, NFFT)
    stock = StockSTFT(dev)
    canon = [min(int(v), 1024) for v in make_batch(seed=1234)["mel_lens"]]
    res = {"tool": "tools/bench_griffinlim.py", "iterations": ITERS, "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "steps": a.steps, "warmup": a.warmup, "shapes": {}}
    for name, lens in (("canonical_B16", canon), ("single_T870", [870])):
        B, Fmax = len(lens), max(lens)
        rs = np.random.RandomState(5)
        env = 2.0 / (1.0 + np.arange(513) / 30.0)
        mag = torch.from_numpy((rs.rand(B, 513, Fmax) * env[None, :, None]).astype(np.float32)).to(dev)
        ang = torch.from_numpy(rs.uniform(-np.pi, np.pi, (B, 513, Fmax)).astype(np.float32)).to(dev)
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        nat_ms, nat = timed(lambda: audio.griffin_lim(mag, stft, ITERS, angles=ang, lens=lens_d if B > 1 else None), a.steps, a.warmup)
        # gl_iter_kernel alone: ITERS back-to-back launches on the same frame buffers
        ws = stft._workspace(mag, "magnitude")
        Y, magT = K.istft_frames(mag, ang, ws, lens_d, want_magT=True)
        Y2 = torch.empty_like(Y)

        def iters():
            for _ in range(ITERS):
                K.griffinlim_iter(Y, magT, ws, Y2, lens_d)
        loop_ms, _ = timed(iters, a.steps, a.warmup)
        loop_ms /= ITERS
        k_us = kernel_us(iters, "gl_iter_kernel")
        it_ms = k_us / 1e3 if k_us else loop_ms
        ssteps = max(1, min(a.steps, 3))
        with torch.no_grad():
            st_ms, _ = timed(lambda: [stock.griffin_lim(mag[b:b + 1, :, :F], ang[b:b + 1, :, :F], ITERS) for b, F in enumerate(lens)], ssteps, 1)
            stp_ms, _ = timed(lambda: stock.griffin_lim(mag, ang, ITERS), ssteps, 1)
            diffs = [rel_l2(nat[b:b + 1, :HOP * (F - 1)], stock.griffin_lim(mag[b:b + 1, :, :F], ang[b:b + 1, :, :F], ITERS)) for b, F in enumerate(lens)]
        frames = sum(lens)
        audio_s = sum(HOP * (F - 1) for F in lens) / SR
        gbytes = frames * BYTES_PER_FRAME / 1e9
        res["shapes"][name] = {
            "B": B, "frames": frames, "max_frames": Fmax, "audio_s": round(audio_s, 2),
            "native": {"ms": round(nat_ms, 3), "audio_s_per_s": round(audio_s / (nat_ms / 1e3), 1),
                       "iter_kernel_us": round(k_us, 1) if k_us else None, "iter_loop_us": round(loop_ms * 1e3, 1),
                       "iter_bytes_mb": round(gbytes * 1e3, 2),
                       "iter_tb_per_s": round(gbytes / it_ms, 3), "frac_of_8TBps": round(gbytes / it_ms / PEAK_TBS, 3)},
            "stock_torch_padded_batch": {"ms": round(stp_ms, 3), "audio_s_per_s": round(audio_s / (stp_ms / 1e3), 1)},
            "stock_torch_per_utterance": {"ms": round(st_ms, 3), "audio_s_per_s": round(audio_s / (st_ms / 1e3), 1)},
            "speedup_vs_padded_batch": round(stp_ms / nat_ms, 2), "speedup_vs_per_utterance": round(st_ms / nat_ms, 2),
            "max_rel_l2_vs_stock": max(diffs)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
