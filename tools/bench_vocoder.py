"""HiFi-GAN V1 generator: the native vocoder (csrc/vocoder.hip through vocoder.Generator) against a stock-torch fp32 forward (F.conv1d /
F.conv_transpose1d of tests/hifigan_restate.py on the same folded weights and the same input), same GPU, same process.  Prints ONE JSON
line.  Shapes: the padded canonical batch (B = 16, synthetic.make_batch()'s mel_lens, padded to 1024 frames - what synth_samples hands
the vocoder) and one 870-frame utterance (LJSpeech's longest, synthesize.py --mode single).  Per shape: warm median ms over HIP events,
audio-seconds per second, algorithmic TFLOP/s and its fraction of 416.7 TF (the bf16 pipe / 6), per-stage ms, max-abs difference.

    python tools/bench_vocoder.py [--steps 20] [--warmup 5] [--out profiles/vocoder_bench.json] [--once]
--once runs a single native forward of the canonical batch and exits (for a kernel-trace profile of one forward).

    python tools/bench_vocoder.py --ragged [--repeats 3] [--parent parent.json] [--out profiles/vocoder_ragged_bench.json]
--ragged measures the length-aware forward (Generator.forward(mel, lens)) instead, V1 at the canonical lengths: (a) the dense
[16, 80, 1024] forward, (c) the same batch with lens, (d) the sum of 16 native B = 1 calls on the unpadded mels, and the dense
B = 1 x 870 forward, and the same batch with every length 0 (each of the 78 grids dispatched, every workgroup returning at once: what
the skipped tiles of a ragged forward still cost, scaled by their share); each the warm median over --steps, repeated --repeats times (spread = the largest gap between repeats of a case).
--dense-only keeps to the cases that need no `lens` (so the same tool runs on a checkout that predates it); --parent FILE embeds such a
run's figures as (b).  Also printed: the share of the conv workgroups (128-row tiles x column blocks, summed over layers) that a
ragged forward does not skip.

    python tools/bench_vocoder.py --precision fp16 [--ragged] [--repeats 3] [--out profiles/vocoder_half_bench.json]
--precision fp16 measures the half-precision inference mode (g(mel, precision="fp16") on a Generator, csrc/vocoder_h.hip) in one run
at both shapes: the native fp16 mode, the native fp32 mode and stock torch fp16 (the restatement's F.conv1d / F.conv_transpose1d on the
same folded weights after .half(), MIOpen), interleaved and repeated like --ragged; with --ragged also both native modes with `lens` on
the canonical batch.  Reported: the ratios, the per-stage ms of both native modes and the wav error (max, rms) of both half paths
against the native fp32 output.

--quality (opt-in; the plain and the --precision fp16 report) adds a "quality" entry per shape: the mel-cepstral distortion
(ctts_amd.metrics, MFCC-style: the DCT of this project's log-mel, not WORLD / SPTK mel-cepstra) of each native output, its log-mel
re-extracted by `TacotronSTFT`, against the input mel's own cepstra frame by frame (align="none"), and with --precision fp16 of the fp16
output against the fp32 output (`compare_wavs`).  The weights here are random, so the first figure says what the network does to a
mel, not how a trained vocoder sounds; the second is the distance between the two modes, and comes with the sample-aligned waveform
metrics of the fp16 output against the fp32 output (`waveform_metrics`: STOI, ESTOI, SI-SDR, multi-resolution STFT distances; corpus
means).  The mels here are synthetic, so there is no recording to take those against.  Without the flag the output is unchanged."""
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


def quality(view, wavs):
    """view [B,80,T] (the input mel), wavs {name: [B,1,256 T]} -> {name: MCD dB against the input mel (path_len-weighted)}, plus the
    MCD between the first two outputs when there are two; frame i against frame i"""
    from ctts_amd import audio, metrics as M
    stft = audio.TacotronSTFT(1024, HOP, 1024, 80, SR, 0, 8000).to(view.device)
    mel_in = view.float().contiguous()
    out = {}
    for name, w in wavs.items():
        mel, frames, _ = M.wav_features(w[:, 0], None, stft)
        out[f"{name}_mcd_db_vs_input_mel"] = round(M.summarize(M.compare_mels(mel_in, None, mel, frames, align="none"))["mcd_db"].item(), 4)
    names = list(wavs)
    if len(names) >= 2:
        r = M.summarize(M.compare_wavs(wavs[names[0]][:, 0], None, wavs[names[1]][:, 0], None, stft, align="none"))
        out[f"{names[1]}_vs_{names[0]}"] = {"mcd_db": round(r["mcd_db"].item(), 5), "lf0_rmse_cents": r["lf0_rmse_cents"].item(),
                                           "vuv_error": r["vuv_error"].item(), "n_voiced": int(r["n_voiced"].item())}
        # the sample-aligned waveform metrics between the two modes (the mels here are synthetic: there is no recording to compare with)
        wm = M.summarize_waveform(M.waveform_metrics(wavs[names[0]][:, 0], wavs[names[1]][:, 0], None, SR))
        out[f"{names[1]}_vs_{names[0]}"]["waveform"] = {k: wm[k]["mean"] for k in ("stoi", "estoi", "si_sdr", "sc", "log_mag", "lsd_db")}
    return out


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


def live_workgroup_share(h, lens, T):
    """(not skipped, launched) workgroups of the generator's conv layers for a batch of `lens` padded to T: csrc/vocoder.hip's grid is
    ceil(Mrows / 128) row tiles x ceil(N / BN) column blocks per utterance, and a tile at or beyond its utterance's rows returns"""
    def blocks(n):
        bn = 128 if n % 128 == 0 else (64 if n % 64 == 0 else 32)
        return -(-n // bn)
    layers = [(1, 0, blocks(h["upsample_initial_channel"]))]          # (rows per frame, extra rows of the polyphase range, blocks)
    s, c = 1, h["upsample_initial_channel"]
    for u, k in zip(h["upsample_rates"], h["upsample_kernel_sizes"]):
        pad = (k - u) // 2
        c //= 2
        layers.append((s, (pad + u - 1) // u - pad // u, blocks(u * c)))
        s *= u
        layers += [(s, 0, blocks(c))] * (6 * len(h["resblock_kernel_sizes"]))
    live = sum(-(-(n * s + e) // 128) * nb for s, e, nb in layers for n in lens if n > 0)
    return live, sum(-(-(T * s + e) // 128) * nb * len(lens) for s, e, nb in layers)


def ragged_main(a, dev, g, mel_lens):
    gen = torch.Generator().manual_seed(0)
    mel = (torch.randn(16, 1024, 80, generator=gen) * 2 - 5).to(dev)
    single = (torch.randn(1, 870, 80, generator=gen) * 2 - 5).to(dev)
    view, sview = mel.transpose(1, 2), single.transpose(1, 2)
    lens = torch.tensor(mel_lens, dtype=torch.int32, device=dev)
    alone = [view[b:b + 1, :, :n] for b, n in enumerate(mel_lens)]
    cases = {"a_dense_B16_T1024": lambda cb: g._forward(view), "dense_single_T870": lambda cb: g._forward(sview)}
    if not a.dense_only:
        cases["c_ragged_B16_T1024"] = lambda cb: g._forward(view, lens=lens)
        cases["d_sum_of_16_single_calls"] = lambda cb: [g._forward(m) for m in alone][-1]
        empty = torch.zeros_like(lens)
        cases["all_empty_B16_T1024"] = lambda cb: g._forward(view, lens=empty)
    res = {"tool": "tools/bench_vocoder.py --ragged" + (" --dense-only" if a.dense_only else ""),
           "network": "HiFi-GAN V1 (hifigan/config.json), folded weights",
           "arithmetic": "split (exact 3-way bf16, 6 MFMA terms)" if K.BF16_SPLIT else "fp32 MFMA",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "mel_lens": mel_lens, "valid_frames": sum(mel_lens), "padded_frames": 16 * 1024, "cases": {}}
    runs = {k: [] for k in cases}
    with torch.no_grad():
        for _ in range(a.repeats):                       # interleaved: a drift of the box shows up as spread, not as a difference
            for k, fn in cases.items():
                runs[k].append(timed(fn, a.steps, a.warmup, False)[0])
    for k, v in runs.items():
        res["cases"][k] = {"ms": round(statistics.median(v), 3), "repeats_ms": [round(x, 3) for x in v], "spread_ms": round(max(v) - min(v), 3)}
    if a.parent:
        with open(a.parent) as f:
            par = json.loads(f.readline())
        res["cases"]["b_parent_dense_B16_T1024"] = par["cases"]["a_dense_B16_T1024"]
        res["cases"]["parent_dense_single_T870"] = par["cases"]["dense_single_T870"]
    if not a.dense_only:
        live, total = live_workgroup_share(V1, mel_lens, 1024)
        ms = {k: v["ms"] for k, v in res["cases"].items()}
        res["frame_share"] = round(sum(mel_lens) / (16 * 1024), 4)
        res["live_workgroup_share"] = round(live / total, 4)
        res["ragged_over_dense"] = round(ms["c_ragged_B16_T1024"] / ms["a_dense_B16_T1024"], 4)
        res["skipped_workgroups_ms_estimate"] = round((1 - live / total) * ms["all_empty_B16_T1024"], 3)
        res["ragged_over_sum_of_singles"] = round(ms["c_ragged_B16_T1024"] / ms["d_sum_of_16_single_calls"], 4)
        with torch.no_grad():                            # per stage (events between the stages, one more pass): where the ratio is lost
            st_a = timed(lambda cb: g._forward(view, cb), a.steps, a.warmup, True)[1]
            st_c = timed(lambda cb: g._forward(view, cb, lens=lens), a.steps, a.warmup, True)[1]
        res["stage_ms"] = {k: {"dense": st_a[k], "ragged": st_c[k], "ratio": round(st_c[k] / st_a[k], 3)} for k in st_a}
        with torch.no_grad():                            # what the tool times is what the tests hold: bit-equal to the B = 1 calls
            wav = g(view, lens=lens)
            res["bit_equal_to_single_calls"] = all(torch.equal(wav[b, 0, :HOP * n], g(alone[b])[0, 0]) for b, n in enumerate(mel_lens))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def half_main(a, dev, g, mel_lens):
    gen = torch.Generator().manual_seed(0)
    mels = {"canonical_B16_T1024": (torch.randn(16, 1024, 80, generator=gen) * 2 - 5).to(dev),
            "single_T870": (torch.randn(1, 870, 80, generator=gen) * 2 - 5).to(dev)}
    if a.once:                                           # one fp16 forward of the canonical batch (for a kernel-trace profile)
        with torch.no_grad():
            g(mels["canonical_B16_T1024"].transpose(1, 2), precision="fp16")
            g(mels["canonical_B16_T1024"].transpose(1, 2), precision="fp16")     # the second one runs on the cached pack
        torch.cuda.synchronize()
        print(json.dumps({"once": "canonical_B16_T1024", "precision": "fp16"}))
        return
    W16 = R.fold_state_dict(g.state_dict(), dtype=torch.float16, device=dev)
    lens = torch.tensor(mel_lens, dtype=torch.int32, device=dev)
    res = {"tool": "tools/bench_vocoder.py --precision fp16" + (" --ragged" if a.ragged else ""),
           "network": "HiFi-GAN V1 (hifigan/config.json), folded weights",
           "fp32_arithmetic": "split (exact 3-way bf16, 6 MFMA terms)" if K.BF16_SPLIT else "fp32 MFMA",
           "fp16_arithmetic": "fp16 weights and activations, v_mfma_f32_32x32x16_f16, fp32 accumulation (include/ctts.h)",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "shapes": {}}
    fpf = R.flops_per_frame(V1)
    for name, m in mels.items():
        view = m.transpose(1, 2)
        B, _, T = view.shape
        half_view = view.contiguous().half()             # a dense [B, 80, T] half mel: stock torch at its best, no re-layout per call
        cases = {"native_fp16": lambda cb: g._forward(view, precision="fp16"),
                 "native_fp32": lambda cb: g._forward(view, precision="fp32"),
                 "stock_torch_fp16": lambda cb: R.generator_forward(W16, V1, half_view)}
        if a.ragged and B > 1:
            cases["native_fp16_ragged"] = lambda cb: g._forward(view, lens=lens, precision="fp16")
            cases["native_fp32_ragged"] = lambda cb: g._forward(view, lens=lens, precision="fp32")
        runs = {k: [] for k in cases}
        with torch.no_grad():
            for _ in range(a.repeats):                   # interleaved: a drift of the box shows up as spread, not as a difference
                for k, fn in cases.items():
                    runs[k].append(timed(fn, a.steps, a.warmup, False)[0])
            st16 = timed(lambda cb: g._forward(view, cb, precision="fp16"), a.steps, a.warmup, True)[1]
            st32 = timed(lambda cb: g._forward(view, cb, precision="fp32"), a.steps, a.warmup, True)[1]
            ref = g(view, precision="fp32").double()
            err = {}
            for k, out in (("native_fp16", g(view, precision="fp16")), ("stock_torch_fp16", R.generator_forward(W16, V1, half_view))):
                e = out.double() - ref
                err[k] = {"max": e.abs().max().item(), "rms": e.pow(2).mean().sqrt().item(), "finite": bool(torch.isfinite(out).all())}
        flop, audio_s = fpf * B * T, B * T * HOP / SR
        ms = {k: statistics.median(v) for k, v in runs.items()}
        sh = {"B": B, "T": T, "tflop": round(flop / 1e12, 3), "wav_std": round(ref.std().item(), 4), "cases": {}}
        for k, v in runs.items():
            sh["cases"][k] = {"ms": round(ms[k], 3), "repeats_ms": [round(x, 3) for x in v], "spread_ms": round(max(v) - min(v), 3),
                              "audio_s_per_s": round(audio_s / (ms[k] / 1e3), 1), "tflops": round(flop / ms[k] / 1e9, 1)}
        sh["fp32_over_fp16"] = round(ms["native_fp32"] / ms["native_fp16"], 3)
        sh["stock_fp16_over_native_fp16"] = round(ms["stock_torch_fp16"] / ms["native_fp16"], 3)
        if "native_fp16_ragged" in ms:
            sh["fp32_over_fp16_ragged"] = round(ms["native_fp32_ragged"] / ms["native_fp16_ragged"], 3)
            sh["valid_frames"], sh["padded_frames"] = sum(mel_lens), B * T
        sh["stage_ms"] = {k: {"fp16": st16[k], "fp32": st32[k], "ratio": round(st32[k] / st16[k], 3)} for k in st16}
        sh["wav_error_vs_native_fp32"] = err
        if a.quality:
            with torch.no_grad():
                sh["quality"] = quality(view, {"native_fp32": g(view, precision="fp32"), "native_fp16": g(view, precision="fp16")})
        res["shapes"][name] = sh
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--quality", action="store_true", help="add the mel-cepstral distortion of the outputs (see the module docstring)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = v1_generator(dev)
    W = R.fold_state_dict(g.state_dict(), dtype=torch.float32, device=dev)
    batch = make_batch(seed=1234)
    mel_lens = [int(v) for v in batch["mel_lens"]]
    if a.precision == "fp16":
        return half_main(a, dev, g, mel_lens)
    if a.ragged:
        return ragged_main(a, dev, g, mel_lens)
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
        if a.quality:
            res["shapes"][name]["quality"] = quality(view, {"native_fp32": nat})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
