"""DeepSpeaker speaker embeddings on the device (csrc/speaker.hip through ctts_amd.speaker) against a stock-torch formulation of the same
chain on the same device and weights, timed in the same run.  Prints ONE JSON line.

Batch: the canonical 16 speech-like utterances of tools/bench_resample.py at 22.05 kHz.  Weights: the seeded recipe of
tests/speaker_restate.py (the pretrained checkpoint is not available).  Timing: warm-up, then the median over HIP events around
back-to-back calls (tools/bench_pitch_features.timed).
Native: span + fbank (two launches), the conv stack (28 convolutions + head on the native features), the whole call, and each stage alone.
Stock torch: the front end per utterance with torch.quantile, unfold, torch.fft.rfft and a filterbank matmul (it reads the span back
to the host, as the reference does); the conv stack as F.conv2d (MIOpen) on the same BN-folded weights with explicit TF 'same' padding,
NCHW, each stage alone as well.  Both conv stacks run on the native features, so their errors against the float64 restatement of
tests/speaker_restate.py are comparable; each front end is compared on its own output.  The conv stack's FLOP/s are set against the
157.3 TFLOP/s of the fp32 matrix pipe (v_mfma_f32_32x32x2_f32), the pipe the kernel uses.  No speed-up was fixed in advance.
PARITY with the TF model and python_speech_features is UNPINNED (neither is installed where this project is built).

    python tools/bench_speaker.py [--steps 20] [--warmup 3] [--out profiles/speaker_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import kernels as K  # noqa: E402
from ctts_amd import speaker as S  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402
from bench_pitch_features import timed  # noqa: E402
from bench_resample import speechlike  # noqa: E402
import speaker_restate as R  # noqa: E402

FP32_MATRIX_FLOPS = 157.3e12


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def conv_flops(B):
    """(total, per stage) multiply-adds x 2 of the 28 convolutions"""
    per, H, W, cin = [], 160, 64, 1
    for c in S.STAGES:
        H, W = -(-H // 2), -(-W // 2)
        per.append(2.0 * B * H * W * c * (25 * cin + 6 * 9 * c))
        cin = c
    return sum(per), per


class StockTorch:
    def __init__(self, emb, dev):
        self.convs = [(w.permute(3, 2, 0, 1).contiguous(), b) for w, b in emb._convs]
        self.affine = emb._affine
        self.fb = torch.from_numpy(R.filterbank()).float().to(dev)
        self.dev = dev

    def front(self, wav, lens):
        out = torch.zeros(len(lens), 160, 64, device=self.dev)
        for i, n in enumerate(lens):
            x = wav[i, :n]
            a = x.abs()
            idx = (a.double() > torch.quantile(a.double(), 0.95)).nonzero()
            if idx.numel() == 0 or int(idx[-1]) - int(idx[0]) < 1:
                continue
            s = x[int(idx[0]):int(idx[-1])]
            y = torch.cat([s[:1], s[1:] - 0.97 * s[:-1]])
            nf = R.n_frames(y.numel())
            frames = F.pad(y, (0, (nf - 1) * R.STEP + R.FRAME - y.numel())).unfold(0, R.FRAME, R.STEP)
            spec = torch.fft.rfft(frames, R.NFFT)
            feat = ((spec.real ** 2 + spec.imag ** 2) / R.NFFT) @ self.fb.T
            feat = torch.where(feat == 0, torch.full_like(feat, R.EPS), feat)
            feat = (feat - feat.mean(1, keepdim=True)) / feat.std(1, unbiased=False, keepdim=True).clamp(min=1e-12)
            r = max(nf - 160, 0) // 2
            rows = feat[r:r + 160]
            out[i, :rows.shape[0]] = rows
        return out

    def stage(self, x, i):
        """NCHW in and out"""
        convs = self.convs[7 * i:7 * i + 7]
        _, pt, pb = R.same_pads(x.shape[2], 5, 2)
        _, pl, pr = R.same_pads(x.shape[3], 5, 2)
        x = F.conv2d(F.pad(x, (pl, pr, pt, pb)), convs[0][0], convs[0][1], stride=2).clamp(0, 20)
        for j in range(3):
            (wa, ba), (wb, bb) = convs[1 + 2 * j], convs[2 + 2 * j]
            y = F.conv2d(x, wa, ba, padding=1).clamp(0, 20)
            x = (F.conv2d(y, wb, bb, padding=1).clamp(0, 20) + x).clamp(0, 20)
        return x

    def stack(self, fb, return_stages=False):
        x, stages = fb[:, None], []
        for i in range(4):
            x = self.stage(x, i)
            stages.append(x)
        z = x.permute(0, 2, 3, 1).reshape(x.shape[0], x.shape[2], -1).mean(1) @ self.affine[0] + self.affine[1]
        emb = z / z.norm(dim=1, keepdim=True).clamp(min=1e-12)
        return (emb, stages) if return_stages else emb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speaker_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = [min(int(v), 1024) for v in make_batch(seed=1234)["mel_lens"]]
    sigs = [speechlike(256 * f, 22050, 500 + i) for i, f in enumerate(frames)]
    lens = [len(s) for s in sigs]
    B, N = len(sigs), max(lens)
    host = np.zeros((B, N), np.float32)
    for i, s in enumerate(sigs):
        host[i, :lens[i]] = s
    wav = torch.from_numpy(host).to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    weights = R.make_weights()
    emb = S.DeepSpeakerEmbedder(weights, dev)
    stock = StockTorch(emb, dev)

    def front():
        first, last, nf, valid = K.speaker_span(wav, lens_d)
        return K.speaker_fbank(wav, first, last, valid, emb._bins, 160, centre=True)

    note("native front end")
    ms_front, fb = timed(front, a.steps, a.warmup)
    note("native conv stack")
    ms_stack, (e_nat, st_nat) = timed(lambda: emb.forward_features(fb, return_stages=True), a.steps, a.warmup)
    ms_whole, res = timed(lambda: emb(wav, lens_d), a.steps, a.warmup)
    note("stock front end")
    ms_s_front, fb_s = timed(lambda: stock.front(wav, lens), max(a.steps // 4, 3), 1, inner=2)
    note("stock conv stack (MIOpen picks its kernels in the warm-up)")
    ms_s_stack, (e_st, st_st) = timed(lambda: stock.stack(fb, return_stages=True), a.steps, a.warmup)
    per_stage = []
    total, per_flops = conv_flops(B)
    x_n, x_s = fb.unsqueeze(-1), fb[:, None]
    for i in range(4):
        note(f"stage {i + 1}")
        ms_n, y_n = timed(lambda: emb.stage(x_n, i), a.steps, a.warmup)
        ms_s, y_s = timed(lambda: stock.stage(x_s, i), a.steps, a.warmup)
        per_stage.append({"stage": i + 1, "out_nhwc": list(y_n.shape), "gflop": round(per_flops[i] / 1e9, 2), "native_ms": round(ms_n, 4),
                          "stock_torch_ms": round(ms_s, 4), "speedup": round(ms_s / ms_n, 3),
                          "native_tflops": round(per_flops[i] / (ms_n * 1e-3) / 1e12, 2),
                          "native_fraction_of_fp32_matrix_peak": round(per_flops[i] / (ms_n * 1e-3) / FP32_MATRIX_FLOPS, 4)})
        x_n, x_s = y_n, y_s
    note("float64 restatement on the host")
    feats = [R.features(s) for s in sigs]
    fb64 = torch.stack([f[0] for f in feats])
    e64, st64, _ = R.rescnn(weights, fb.cpu().double())                      # both conv stacks ran on the native features
    err = {"native_fbank": float((fb.cpu().double() - fb64).abs().max()), "stock_torch_fbank": float((fb_s.cpu().double() - fb64).abs().max()),
           "native_stage4": float((st_nat[3].cpu().double() - st64[3]).abs().max()),
           "stock_torch_stage4": float((st_st[3].permute(0, 2, 3, 1).cpu().double() - st64[3]).abs().max()),
           "native_embedding": float((e_nat.cpu().double() - e64).abs().max()), "stock_torch_embedding": float((e_st.cpu().double() - e64).abs().max())}
    span_ok = res["first"].cpu().tolist() == [f[1] for f in feats] and res["last"].cpu().tolist() == [f[2] for f in feats]
    out = {"tool": "tools/bench_speaker.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "batch": {"utterances": B, "frames": frames, "audio_s": round(sum(lens) / 22050.0, 2), "fbank_frames": res["n_frames"].cpu().tolist()},
           "span_fbank_ms": round(ms_front, 4), "conv_stack_ms": round(ms_stack, 4), "whole_call_ms": round(ms_whole, 4),
           "stock_torch_front_end_ms": round(ms_s_front, 4), "stock_torch_conv_stack_ms": round(ms_s_stack, 4),
           "speedup_front_end": round(ms_s_front / ms_front, 3), "speedup_conv_stack": round(ms_s_stack / ms_stack, 3),
           "conv_stack_gflop": round(total / 1e9, 2), "conv_stack_tflops": round(total / (ms_stack * 1e-3) / 1e12, 2),
           "conv_stack_fraction_of_fp32_matrix_peak": round(total / (ms_stack * 1e-3) / FP32_MATRIX_FLOPS, 4),
           "stock_torch_conv_stack_tflops": round(total / (ms_s_stack * 1e-3) / 1e12, 2),
           "utterances_per_s": round(B / (ms_whole * 1e-3), 1), "per_stage": per_stage, "max_abs_error_vs_float64": err,
           "span_equals_restatement": bool(span_ok),
           "note": "parity with the TF model and python_speech_features unpinned (neither is installed; seeded random weights): both sides "
                   "are pinned against the float64 restatement in tests/speaker_restate.py; no speed-up was fixed in advance",
           "steps": a.steps, "warmup": a.warmup}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
