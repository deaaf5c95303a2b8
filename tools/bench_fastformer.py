"""block_type "fastformer" against "transformer_fs2" on one MI355X, same process, same batch.

  python tools/bench_fastformer.py [--steps 20] [--warmup 5] [--out FILE]

The canonical B = 16 batch with mel frames capped at 1000 (the fastformer / conformer decoders crop to max_seq_len = 1000 in training, so
both models see the same frames).  Prints ONE JSON line:
  train_{fastformer,fs2}_ms, ..._valid_mel_frames_per_s   captured train step (hipGraph replay, TrainStep as bench.py builds it)
  infer_{fastformer,fs2}_ms                                free-running inference forward (no targets, eval mode)
  kernels                                                  each csrc/fastformer.hip launch at the decoder's shape: us and TB/s
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ctts_amd  # noqa: E402
from ctts_amd import kernels as K  # noqa: E402
from ctts_amd.configs import get_configs  # noqa: E402
from ctts_amd.loss import CompTransTTSLoss, ScheduledOptim  # noqa: E402
from ctts_amd.synthetic import make_batch, to_device, as_model_args  # noqa: E402
from ctts_amd.trainer import TrainStep  # noqa: E402

DEV = torch.device("cuda", 0)


def _time(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def bench_block(block, batch, steps, warmup):
    pre, mc, tc = get_configs()
    mc["block_type"] = block
    torch.manual_seed(1234)
    model = ctts_amd.CompTransTTS(pre, mc, tc).to(DEV).train()
    loss_fn, optim = CompTransTTSLoss(pre, mc, tc).to(DEV), ScheduledOptim(model, tc, mc, 50000, capturable=True)
    step = TrainStep(model, loss_fn, optim, as_model_args(batch), world=1, use_graph=True)
    step.capture(warmup=2)
    train_ms = _time(step, steps, warmup)
    loss = float(step.loss_val)
    model.eval()
    args = list(as_model_args(batch))
    for i in (4, 5, 6, 7, 8, 9):          # mels, mel_lens, max_mel_len, p / e / d targets: free-running inference
        args[i] = None

    def infer():
        with torch.no_grad():
            model(*args)
    infer_ms = _time(infer, max(3, steps // 2), 2)
    del step, model, optim
    torch.cuda.empty_cache()
    return train_ms, infer_ms, loss


def bench_kernels(B, T, steps):
    H, C = 128, 256
    M = B * T
    g = torch.Generator(device=DEV).manual_seed(0)
    s = torch.randn(M, H, device=DEV, generator=g)
    V, X, dY = (torch.randn(M, C, device=DEV, generator=g) for _ in range(3))
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    lens[1::2] = T * 3 // 4
    rs = torch.ones(M, device=DEV)
    p, st = K.fastformer_pool_fwd(s, V, lens, B, T, H, 2 ** 0.5)
    dp = torch.randn(B, C, device=DEV, generator=g)
    f = 4.0
    cases = {
        # name: (callable, bytes moved: the [M, C] / [M, H] streams each launch reads or writes once)
        "pool_fwd": (lambda: K.fastformer_pool_fwd(s, V, lens, B, T, H, 2 ** 0.5), f * (M * H + M * C)),
        "pool_bwd": (lambda: K.fastformer_pool_bwd(dp, p, st, s, V, lens, B, T, H, 2 ** 0.5, dV_in=dY), f * (2 * M * H + 3 * M * C)),
        "bcast": (lambda: K.fastformer_bcast(X, p, B, T), f * 2 * M * C),
        "bcast_bwd": (lambda: K.fastformer_bcast_bwd(dY, X, p, B, T, dY2=V), f * 4 * M * C),
        "resdrop": (lambda: K.fastformer_resdrop(X, V, rs, 0.2, None, 0), f * 3 * M * C),
    }
    out = {}
    for name, (fn, nbytes) in cases.items():
        us = _time(fn, steps, 3) * 1e3
        out[name] = {"us": round(us, 2), "TB_per_s": round(nbytes / us / 1e6, 2), "MB": round(nbytes / 1e6, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batch = to_device(make_batch(None, seed=1234, max_mel_cap=1000), DEV)
    valid = int(batch["mel_lens"].sum())
    res = {"batch": {"B": int(batch["mel_lens"].numel()), "T_mel": int(batch["max_mel_len"]), "valid_mel_frames": valid}}
    for block, tag in (("fastformer", "fastformer"), ("transformer_fs2", "fs2")):
        tr, inf, loss = bench_block(block, batch, a.steps, a.warmup)
        res[f"train_{tag}_ms"] = round(tr, 3)
        res[f"train_{tag}_valid_mel_frames_per_s"] = round(valid / tr * 1e3, 1)
        res[f"infer_{tag}_ms"] = round(inf, 3)
        res[f"loss_{tag}"] = loss
    res["fastformer_over_fs2_throughput"] = round(res["train_fastformer_valid_mel_frames_per_s"] / res["train_fs2_valid_mel_frames_per_s"], 4)
    res["kernels"] = bench_kernels(16, int(batch["max_mel_len"]), 50)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
