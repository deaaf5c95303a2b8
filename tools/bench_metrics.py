"""Objective evaluation on the device (csrc/metrics.hip through ctts_amd.metrics): the three kernels and `compare_mels` on the canonical
batch, against a stock-torch anti-diagonal DTW on the same device in the same run and the numpy restatement (tests/metrics_restate.py)
of one pair on the host.  Prints ONE JSON line.

Batch: 16 reference utterances with the canonical mel lengths (synthetic.make_batch()'s mel_lens, capped at 1024 frames), smooth random
log-mels; the synthetic side has those lengths scaled by a fixed-seed factor in [0.9, 1.1] and is a time-warped, noisy copy of the
reference, with F0 contours to match.  Reported: median time per call over HIP events around back-to-back calls for the cepstrum, the
DTW (both launches), the path sums and the whole of `compare_mels`; the device time of each kernel from a torch.profiler trace; the
stock-torch DTW (torch.cdist, then one batched step per anti-diagonal on the skewed cost tensor - accumulated cost only, no path); the
host time of the restatement for the batch's median pair; and what the backtrack - a single lane following dependent loads - costs:
two single pairs of 2047 x 2047 frames with the same sweep and paths of 2047 and 4091 pairs, the difference per step, and from it the
backtrack's share of the sweep kernel on the canonical batch's longest pair.
No speed bar is set on these numbers: they are what was measured.  The MCD is MFCC-style (the DCT of this project's log-mel), NOT
WORLD / SPTK mel-cepstra: parity with those tools is UNPINNED, neither is installed where this project is built.

    python tools/bench_metrics.py [--steps 20] [--warmup 3] [--out profiles/metrics_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import metrics as M  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402
from bench_pitch_features import kernel_us, timed  # noqa: E402
from tests import metrics_restate as R  # noqa: E402

N_MEL, N_COEF = 80, 13


def smooth_mel(rng, F):
    m = np.cumsum(rng.standard_normal((N_MEL, F)), axis=1) * 0.25
    return np.clip(m - 5.0 + 0.5 * rng.standard_normal((N_MEL, 1)), -11.5, 2.0).astype(np.float32)


def stock_dtw_cost(x, y, lx, ly):
    """accumulated DTW cost per pair on stock torch device ops: cdist, the cost tensor skewed so that an anti-diagonal is a row, then one
    batched relaxation per anti-diagonal.  No directions, no path."""
    B, Tx, _ = x.shape
    Ty = y.shape[1]
    dev = x.device
    D = torch.cdist(x, y)                                                   # [B, Tx, Ty]
    nd = Tx + Ty - 1
    i = torch.arange(Tx, device=dev)[None, :]
    j = torch.arange(nd, device=dev)[:, None] - i                          # [nd, Tx]
    inside = (j >= 0) & (j < Ty)
    Dsk = D.gather(2, j.clamp(0, Ty - 1).t()[None].expand(B, Tx, nd)).transpose(1, 2)        # [B, nd, Tx]: Dsk[b, d, i] = D[b, i, d - i]
    valid = inside[None] & (i[None] < lx[:, None, None]) & (j[None] < ly[:, None, None])      # [B, nd, Tx]
    inf = torch.full((B, Tx + 1), float("inf"), device=dev)
    p1, p2 = inf.clone(), inf.clone()                                       # index i + 1; slot 0 is the row above row 0
    last = (lx + ly - 2).clamp(min=0)
    out = torch.zeros(B, device=dev)
    rows = (lx - 1).clamp(min=0).long()[:, None]
    for d in range(nd):
        best = torch.minimum(p2[:, :-1], torch.minimum(p1[:, :-1], p1[:, 1:]))
        if d == 0:
            best = torch.zeros_like(best)
        cur = torch.where(valid[:, d], Dsk[:, d] + best, inf[:, 1:])
        out = torch.where(last == d, cur.gather(1, rows)[:, 0], out)
        p2 = p1
        p1 = torch.cat([inf[:, :1], cur], 1)
    return torch.where((lx > 0) & (ly > 0), out, torch.zeros_like(out))


def corner_pair(L, K, dev):
    """two L-frame sequences whose only zero-cost path has 2 L - 3 pairs: along row 0, one diagonal step pair, down the last column"""
    g = torch.Generator().manual_seed(3)
    a0, a1, z = (torch.randn(K, generator=g) for _ in range(3))
    x = torch.stack([a0, a1] + [z] * (L - 2))
    y = torch.stack([a0] * (L - 2) + [a1, z])
    return x[None].to(dev).contiguous(), y[None].to(dev).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1234)
    ref_lens = [min(int(v), 1024) for v in make_batch(seed=1234)["mel_lens"]]
    syn_lens = [max(2, int(round(n * f))) for n, f in zip(ref_lens, rng.uniform(0.9, 1.1, len(ref_lens)))]
    B, Fr, Fs = len(ref_lens), max(ref_lens), max(syn_lens)
    mel_r, mel_s = np.zeros((B, N_MEL, Fr), np.float32), np.zeros((B, N_MEL, Fs), np.float32)
    f0_r, f0_s = np.zeros((B, Fr), np.float32), np.zeros((B, Fs), np.float32)
    for b, (nr, ns) in enumerate(zip(ref_lens, syn_lens)):
        m = smooth_mel(rng, nr)
        pos = np.clip(np.round(np.linspace(0, nr - 1, ns) + rng.uniform(-1.5, 1.5, ns)), 0, nr - 1).astype(int)
        pos.sort()
        f = 150.0 + 50.0 * np.sin(np.arange(nr) * 0.05 + b)
        f[np.sin(np.arange(nr) * 0.021 + 2 * b) < -0.4] = 0.0
        mel_r[b, :, :nr], f0_r[b, :nr] = m, f
        mel_s[b, :, :ns] = m[:, pos] + 0.3 * rng.standard_normal((N_MEL, ns)).astype(np.float32)
        f0_s[b, :ns] = f[pos] * np.where(f[pos] > 0, 2.0 ** (rng.standard_normal(ns) * 0.02), 1.0)
    t = lambda v: torch.from_numpy(v).to(dev)       # noqa: E731
    mel_r, mel_s, f0_r, f0_s = t(mel_r), t(mel_s), t(f0_r), t(f0_s)
    fr, fs = torch.tensor(ref_lens, dtype=torch.int32, device=dev), torch.tensor(syn_lens, dtype=torch.int32, device=dev)

    cep_ms, cx = timed(lambda: M.mel_cepstrum(mel_r, fr, N_COEF), a.steps, a.warmup)
    cy = M.mel_cepstrum(mel_s, fs, N_COEF)
    dtw_ms, al = timed(lambda: M.dtw(cx, fr, cy, fs), a.steps, a.warmup)
    pm_ms, pm = timed(lambda: M.path_metrics(al["path"], al["path_len"], f0_r, f0_s), a.steps, a.warmup)
    all_ms, res = timed(lambda: M.compare_mels(mel_r, fr, mel_s, fs, f0_r, f0_s, n_coef=N_COEF), a.steps, a.warmup)
    none_ms, _ = timed(lambda: M.compare_mels(mel_r, fr, mel_s, fs, f0_r, f0_s, align="none", n_coef=N_COEF), a.steps, a.warmup)
    kern = {k: kernel_us(fn, k) for k, fn in (("mel_cepstrum_kernel", lambda: M.mel_cepstrum(mel_r, fr, N_COEF)),
                                              ("dtw_cost_kernel", lambda: M.dtw(cx, fr, cy, fs)),
                                              ("dtw_sweep_kernel", lambda: M.dtw(cx, fr, cy, fs)),
                                              ("path_metrics_kernel", lambda: M.path_metrics(al["path"], al["path_len"], f0_r, f0_s)))}
    summary = {k: float(v) for k, v in M.summarize(res).items()}

    stock_ms, stock = timed(lambda: stock_dtw_cost(cx, cy, fr, fs), max(2, a.steps // 5), 1, inner=1)
    stock_rel = float(((stock.double() - al["cost"].double()).abs() / al["cost"].double()).max())

    # the host restatement, one pair: the batch's median reference length
    b = int(np.argsort(ref_lens)[B // 2])
    xh, yh = cx[b, :ref_lens[b]].cpu().numpy(), cy[b, :syn_lens[b]].cpu().numpy()
    t0 = time.perf_counter()
    h_cost, h_path = R.dtw(xh, yh)
    host_ms = (time.perf_counter() - t0) * 1e3

    # the backtrack: same 2047 x 2047 sweep, paths of 2047 and of 4091 pairs
    L = 2047
    g = torch.Generator().manual_seed(5)
    xi = torch.randn(1, L, N_COEF, generator=g).to(dev)
    xc, yc = corner_pair(L, N_COEF, dev)
    n1 = torch.tensor([L], dtype=torch.int32, device=dev)
    short = M.dtw(xi, n1, xi.clone(), n1)
    long_ = M.dtw(xc, n1, yc, n1)
    us_short = kernel_us(lambda: M.dtw(xi, n1, xi.clone(), n1), "dtw_sweep_kernel")
    us_long = kernel_us(lambda: M.dtw(xc, n1, yc, n1), "dtw_sweep_kernel")
    steps = int(long_["path_len"].item()) - int(short["path_len"].item())
    per_step = (us_long - us_short) / steps if us_long and us_short and steps > 0 else None
    # one pair alone, the batch's longest: its sweep kernel and the backtrack's estimated part of it
    bl = int(np.argmax(ref_lens))
    one = lambda: M.dtw(cx[bl:bl + 1], fr[bl:bl + 1], cy[bl:bl + 1], fs[bl:bl + 1])      # noqa: E731
    us_one = kernel_us(one, "dtw_sweep_kernel")
    len_one = int(one()["path_len"].item())

    out = {
        "tool": "tools/bench_metrics.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
        "batch": {"pairs": B, "ref_frames": ref_lens, "syn_frames": syn_lens, "padded": [Fr, Fs], "n_mel": N_MEL, "n_coef": N_COEF,
                  "dtw_cells": int(sum(r * s for r, s in zip(ref_lens, syn_lens))), "path_pairs": int(al["path_len"].sum())},
        "call_us": {"mel_cepstrum_ref": round(cep_ms * 1e3, 1), "dtw": round(dtw_ms * 1e3, 1), "path_metrics": round(pm_ms * 1e3, 1),
                    "compare_mels_dtw": round(all_ms * 1e3, 1), "compare_mels_none": round(none_ms * 1e3, 1)},
        "kernel_us": {k: (round(v, 1) if v else None) for k, v in kern.items()},
        "stock_torch_dtw_cost_only_ms": round(stock_ms, 2), "stock_over_native_dtw": round(stock_ms / dtw_ms, 1),
        "stock_vs_native_cost_max_rel": stock_rel,
        "host_numpy_one_pair": {"frames": [ref_lens[b], syn_lens[b]], "ms": round(host_ms, 1),
                                "cost_rel_vs_device": abs(h_cost - float(al["cost"][b])) / h_cost,
                                "path_len": len(h_path), "device_path_len": int(al["path_len"][b])},
        "backtrack": {"frames": [L, L], "path_pairs": [int(short["path_len"].item()), int(long_["path_len"].item())],
                      "sweep_kernel_us": [round(us_short, 1) if us_short else None, round(us_long, 1) if us_long else None],
                      "us_per_step": round(per_step, 4) if per_step is not None else None,
                      "share_of_short_2047": round(per_step * L / us_short, 3) if per_step is not None else None,
                      "longest_canonical_pair": {"frames": [ref_lens[bl], syn_lens[bl]], "path_pairs": len_one,
                                                 "sweep_kernel_us": round(us_one, 1) if us_one else None,
                                                 "backtrack_share": round(per_step * len_one / us_one, 3) if per_step is not None and us_one else None}},
        "summary": summary,
        "speed_bar": None,
        "note": "no speed bar is set; the stock-torch DTW (cost only, no path) and the host restatement of the same run are the comparison.  "
                "MFCC-style MCD: the DCT of this project's log-mel, NOT WORLD / SPTK mel-cepstra; parity with those tools is UNPINNED "
                "(neither is installed)",
        "steps": a.steps, "warmup": a.warmup,
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
