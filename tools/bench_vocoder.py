"""HiFi-GAN V1 generator: the native vocoder (csrc/vocoder.hip through vocoder.Generator) against a stock-torch fp32 forward (F.conv1d /
F.conv_transpose1d of tests/hifigan_restate.py on the same folded weights and the same input), same GPU, same process.  Prints ONE JSON
line.  Shapes: the padded canonical batch (B = 16, synthetic.make_batch()'s mel_lens, padded to 1024 frames - what synth_samples hands
the vocoder) and one 870-frame utterance (LJSpeech's longest, synthesize.py --mode single).  Per shape: warm median ms over HIP events,
audio-seconds per second, algorithmic TFLOP/s and its fraction of 416.7 TF (the bf16 pipe / 6), per-stage ms, max-abs difference.

    python tools/bench_vocoder.py [--steps 20] [--warmup 5] [--out profiles/vocoder_bench.json] [--once]
--once runs a single native forward of the canonical batch and exits (for a kernel-trace profile of one forward)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402
from ctts_amd import kernels as K  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402
from ctts_amd.vocoder import AttrDict, Generator  # noqa: E402
import hifigan_restate as R  # noqa: E402

V1 = dict(upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], resblock="1")
PEAK_TF = 416.7
HOP, SR = 256, 22050


def v1_generator(dev):
    torch.manual_seed(11)
    g = Generator(AttrDict(V1))
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for name, m in g.named_modules():
            if hasattr(m, "weight_g"):
                m.weight_v.copy_(torch.randn(m.weight_v.shape, generator=gen))
                gain = (m.stride[0] * m.out_channels / m.in_channels) ** 0.5 if name.startswith("ups.") else (0.5 if name == "conv_post" else 1.0)
                m.weight_g.copy_(gain * (0.75 + 0.5 * torch.rand(m.weight_g.shape, generator=gen)))
                m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=gen))
    g.eval()
    g.remove_weight_norm()                      # utils/model.py:66
    return g.to(dev)


def timed(fn, steps, warmup, stages):
    """-> (median ms, {stage: median ms}, last output)"""
    for _ in range(warmup):
        out = fn(None)
    torch.cuda.synchronize()
    tot, per = [], {}
    for _ in range(steps):
        evs = [("start", torch.cuda.Event(enable_timing=True))]
        evs[0][1].record()

        def cb(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append((name, e))
        out = fn(cb if stages else None)
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        torch.cuda.synchronize()
        tot.append(evs[0][1].elapsed_time(end))
        for (_, a), (n, b) in zip(evs, evs[1:]):
            per.setdefault(n, []).append(a.elapsed_time(b))
    return statistics.median(tot), {k: round(statistics.median(v), 3) for k, v in per.items()}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = v1_generator(dev)
    W = R.fold_state_dict(g.state_dict(), dtype=torch.float32, device=dev)
    batch = make_batch(seed=1234)
    mel_lens = [int(v) for v in batch["mel_lens"]]
    gen = torch.Generator().manual_seed(0)
    shapes = {"canonical_B16_T1024": torch.randn(16, 1024, 80, generator=gen) * 2 - 5,
              "single_T870": torch.randn(1, 870, 80, generator=gen) * 2 - 5}
    # the acoustic model's output layout: channel-last [B, T, 80]; the vocoder gets its transposed view (utils/tools.py:342-350)
    for k in shapes:
        shapes[k] = shapes[k].to(dev)
    if a.once:
        with torch.no_grad():
            g(shapes["canonical_B16_T1024"].transpose(1, 2))
        torch.cuda.synchronize()
        print(json.dumps({"once": "canonical_B16_T1024"}))
        return
    fpf = R.flops_per_frame(V1)
    res = {"tool": "tools/bench_vocoder.py", "network": "HiFi-GAN V1 (hifigan/config.json), folded weights",
           "arithmetic": "split (exact 3-way bf16, 6 MFMA terms)" if K.BF16_SPLIT else "fp32 MFMA", "mflop_per_frame": round(fpf / 1e6, 2),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "steps": a.steps, "warmup": a.warmup,
           "canonical_valid_frames": sum(mel_lens), "shapes": {}}
    for name, m in shapes.items():
        view = m.transpose(1, 2)
        B, _, T = view.shape
        with torch.no_grad():
            nat_ms, nat_st, nat = timed(lambda cb: g._forward(view, cb), a.steps, a.warmup, True)
            st_ms, st_st, ref = timed(lambda cb: R.generator_forward(W, V1, view, cb), a.steps, a.warmup, True)
        diff = (nat - ref).abs().max().item()
        flop = fpf * B * T
        audio_s = B * T * HOP / SR
        res["shapes"][name] = {
            "B": B, "T": T, "tflop": round(flop / 1e12, 3),
            "native": {"ms": round(nat_ms, 3), "audio_s_per_s": round(audio_s / (nat_ms / 1e3), 1),
                       "tflops": round(flop / nat_ms / 1e9, 1), "frac_of_416.7TF": round(flop / nat_ms / 1e9 / PEAK_TF, 3), "stage_ms": nat_st},
            "stock_torch_fp32": {"ms": round(st_ms, 3), "audio_s_per_s": round(audio_s / (st_ms / 1e3), 1),
                                 "tflops": round(flop / st_ms / 1e9, 1), "frac_of_416.7TF": round(flop / st_ms / 1e9 / PEAK_TF, 3), "stage_ms": st_st},
            "speedup": round(st_ms / nat_ms, 2), "max_abs_diff": diff}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
