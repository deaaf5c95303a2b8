"""MelGAN generator: the native vocoder (csrc/vocoder.hip through melgan.Generator) against a stock-torch fp32 forward (F.pad reflect /
F.conv1d / F.conv_transpose1d of tests/melgan_restate.py on the same folded weights and the same input, MIOpen), same GPU, same
process, and the two-operand residual tail against the three-launch form (shortcut launch, then block.4 with R=).  Prints ONE JSON line.

    python tools/bench_melgan.py [--steps 20] [--warmup 5] [--repeats 3] [--out profiles/melgan_bench.json]

Shapes: the padded canonical batch (B = 16, synthetic.make_batch()'s mel_lens padded to 1024 frames) dense and with its lengths
(`lens`), and one 870-frame utterance.  Per case the warm median ms over HIP events of --steps forwards, repeated --repeats times with
the cases interleaved (spread = the largest gap between a case's repeats); per shape the audio-seconds per second, algorithmic
TFLOP/s, per-stage ms of the native and the stock forward, and the largest difference between the two outputs.  The weights are the
random recipe of tests/melgan_restate.py, folded."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import kernels as K, melgan  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402
import melgan_restate as MR  # noqa: E402
from bench_vocoder import timed  # noqa: E402

HOP, SR = 256, 22050


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = melgan.Generator()
    g.load_state_dict(MR.recipe_state_dict())
    g.remove_weight_norm()
    g.eval().to(dev)
    W = MR.fold_state_dict(g.state_dict(), dtype=torch.float32, device=dev)
    mel_lens = [int(v) for v in make_batch(seed=1234)["mel_lens"]]
    lens = torch.tensor(mel_lens, dtype=torch.int32, device=dev)
    gen = torch.Generator().manual_seed(0)
    # the acoustic model's output layout: channel-last [B, T, 80]; the vocoder gets its transposed view.  Unit-normal, the scale of
    # mel / ln 10 that the recipe weights were tuned to (wav std about 0.2)
    shapes = {"canonical_B16_T1024": torch.randn(16, 1024, 80, generator=gen).to(dev), "single_T870": torch.randn(1, 870, 80, generator=gen).to(dev)}
    fpf = MR.flops_per_frame()
    res = {"tool": "tools/bench_melgan.py", "network": "MelGAN generator (80, 32, 3), recipe weights, folded",
           "arithmetic": "split (exact 3-way bf16, 6 MFMA terms)" if K.BF16_SPLIT else "fp32 MFMA", "mflop_per_frame": round(fpf / 1e6, 2),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "mel_lens": mel_lens, "valid_frames": sum(mel_lens), "shapes": {}}
    for name, m in shapes.items():
        view = m.transpose(1, 2)
        B, _, T = view.shape
        cases = {"native": lambda cb: g._forward(view, cb),
                 "native_three_launch_tail": lambda cb: g._forward(view, cb, fused_tail=False),
                 "stock_torch_fp32": lambda cb: MR.generator_forward(W, view, cb)}
        if B > 1:
            cases["native_ragged"] = lambda cb: g._forward(view, cb, lens=lens)
            cases["native_ragged_three_launch_tail"] = lambda cb: g._forward(view, cb, lens=lens, fused_tail=False)
        runs = {k: [] for k in cases}
        with torch.no_grad():
            for _ in range(a.repeats):                   # interleaved: a drift of the box shows up as spread, not as a difference
                for k, fn in cases.items():
                    runs[k].append(timed(fn, a.steps, a.warmup, False)[0])
            stages = {k: timed(fn, a.steps, a.warmup, True)[1] for k, fn in cases.items() if "ragged" not in k}
            nat, three, ref = g._forward(view), g._forward(view, fused_tail=False), MR.generator_forward(W, view)
        ms = {k: statistics.median(v) for k, v in runs.items()}
        flop, audio_s = fpf * B * T, B * T * HOP / SR
        sh = {"B": B, "T": T, "tflop": round(flop / 1e12, 4), "wav_std": round(ref.std().item(), 4), "cases": {}}
        for k, v in runs.items():
            valid = sum(mel_lens) / (B * T) if "ragged" in k else 1.0
            sh["cases"][k] = {"ms": round(ms[k], 3), "repeats_ms": [round(x, 3) for x in v], "spread_ms": round(max(v) - min(v), 3),
                              "audio_s_per_s": round(valid * audio_s / (ms[k] / 1e3), 1), "tflops": round(valid * flop / ms[k] / 1e9, 2)}
        sh["speedup_over_stock"] = round(ms["stock_torch_fp32"] / ms["native"], 2)
        sh["three_launch_over_two_operand"] = round(ms["native_three_launch_tail"] / ms["native"], 3)
        if "native_ragged" in ms:
            sh["ragged_three_launch_over_two_operand"] = round(ms["native_ragged_three_launch_tail"] / ms["native_ragged"], 3)
            sh["ragged_over_dense"] = round(ms["native_ragged"] / ms["native"], 3)
            sh["frame_share"] = round(sum(mel_lens) / (B * T), 4)
        sh["stage_ms"] = stages
        sh["max_abs_diff_vs_stock"] = (nat - ref).abs().max().item()
        sh["max_abs_diff_three_launch_vs_two_operand"] = (nat - three).abs().max().item()
        res["shapes"][name] = sh
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
