"""Dataset preparation on the device (csrc/preprocess.hip through ctts_amd.preprocess) against the numpy / scipy restatements of the same
three steps on the host, timed in the same run.  Prints ONE JSON line.

Batch: the canonical 16 speech-like utterances of tools/bench_pitch_features.py (synthetic.make_batch()'s mel lengths capped at 1024,
256 (F - 1) samples each), each with 0.2 s of faint noise in front and behind so that the trim has something to cut; phoneme counts are
the canonical source lengths.  Reported: median time per call over HIP events around back-to-back calls for the trim, the prior and the
outlier-statistics kernels (energy of the batch's own mel kernel), wall time of the whole of `process_batch` (its device-to-host copy of
the results included), and the host times of the restatements: the trim and the IQR filter in numpy (tests/preprocess_restate.py), the
prior as the reference computes it, one `scipy.stats.betabinom` per row, when scipy is importable (else the lgamma closed form).
No speed bar is set on these numbers; the host restatement of the same run is the comparison.  Parity of the trim with librosa is
UNPINNED (librosa is not installed where this project is built): the kernel is pinned against the float64 restatement only.

    python tools/bench_preprocess.py [--steps 20] [--warmup 3] [--out profiles/preprocess_bench.json]"""
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
from ctts_amd import audio, preprocess as PP, pitch_features as PF  # noqa: E402
from ctts_amd.configs import get_configs  # noqa: E402
from ctts_amd.synthetic import CANONICAL_SRC_LENS, make_batch  # noqa: E402
from bench_pitch_features import HOP, SR, speechlike_wave, timed  # noqa: E402
from tests import preprocess_restate as R  # noqa: E402

TOP_DB, FRAME = 23, 1024


def host_time(fn, repeat=3):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, out


def host_prior(src, mel, sf):
    try:
        from scipy.stats import betabinom
    except ImportError:
        return [R.attention_prior(p, m, sf) for p, m in zip(src, mel)], "lgamma closed form (scipy not importable)"
    out = []
    for p, m in zip(src, mel):                              # preprocessor.py:551-560 as called at :409-413
        x = np.arange(m)
        out.append(np.array([betabinom(m, sf * i, sf * (p + 1 - i)).pmf(x) for i in range(1, p + 1)]))
    return out, "scipy.stats.betabinom per row"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = [min(int(v), 1024) for v in make_batch(seed=1234)["mel_lens"]]
    pad = int(0.2 * SR)
    rng = np.random.default_rng(9)
    wavs_h = []
    for b, F in enumerate(frames):
        body = speechlike_wave(HOP * (F - 1) - 2 * pad, 300 + b)
        wavs_h.append(np.concatenate([1e-4 * rng.standard_normal(pad), body, 1e-4 * rng.standard_normal(pad)]).astype(np.float32))
    lens = [len(w) for w in wavs_h]
    B, N = len(lens), max(lens)
    wav_h = np.zeros((B, N), np.float32)
    for b, w in enumerate(wavs_h):
        wav_h[b, :lens[b]] = w
    wav = torch.from_numpy(wav_h).to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    wavs_d = [torch.from_numpy(w).to(dev) for w in wavs_h]
    nph = list(CANONICAL_SRC_LENS)
    stft = audio.TacotronSTFT(1024, 256, 1024, 80, SR, 0, 8000).to(dev)
    pre, _, _ = get_configs()
    pre["preprocessing"]["audio"]["trim_top_db"] = TOP_DB
    PF.prepare(dev)

    trim_ms, (start, end, dur) = timed(lambda: PP.trim_silence(wav, lens_d, TOP_DB, FRAME, HOP), a.steps, a.warmup)
    durs = dur.tolist()
    Ts, Tm = max(nph), max(durs)
    src_d, mel_d = torch.tensor(nph, dtype=torch.int32, device=dev), dur.to(torch.int32)
    prior_buf = torch.empty(B, Ts, Tm, device=dev)
    prior_ms, prior = timed(lambda: PP.attention_prior(src_d, mel_d, 1.0, out=prior_buf), a.steps, a.warmup)
    first = PP.process_batch(wavs_d, nph, stft, pre)
    energy_h = np.zeros((B, Tm), np.float32)
    for b, o in enumerate(first):
        energy_h[b, :durs[b]] = o["energy"]
    energy = torch.from_numpy(energy_h).to(dev)
    out_ms, ostats = timed(lambda: PP.outlier_stats(energy, mel_d), a.steps, a.warmup)

    def whole():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = PP.process_batch(wavs_d, nph, stft, pre)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r
    for _ in range(a.warmup):
        whole()
    pb_ms = statistics.median(whole()[0] for _ in range(a.steps))

    h_trim_ms, h_trim = host_time(lambda: [R.trim_silence(w.astype(np.float64), TOP_DB, FRAME, HOP) for w in wavs_h])
    (h_prior_ms, (h_prior, prior_how)) = host_time(lambda: host_prior(nph, durs, 1.0), repeat=1)
    h_out_ms, h_keep = host_time(lambda: [(R.outlier_keep(energy_h[b, :durs[b]]), R.moments(energy_h[b, :durs[b]])) for b in range(B)])

    got_p = prior.cpu().numpy().astype(np.float64)
    rel = 0.0
    for b in range(B):
        w = h_prior[b]
        big = w >= 1e-30
        rel = max(rel, float((np.abs(got_p[b, :nph[b], :durs[b]][big] - w[big]) / w[big]).max()))
    keep = ostats["keep"].cpu().numpy()
    res = {
        "tool": "tools/bench_preprocess.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
        "batch": {"utterances": B, "audio_s": round(sum(lens) / SR, 2), "frames_after_trim": int(sum(durs)), "phonemes": int(sum(nph)),
                  "prior_shape": [B, Ts, Tm]},
        "trim_us": round(trim_ms * 1e3, 1), "prior_us": round(prior_ms * 1e3, 1), "outlier_stats_us": round(out_ms * 1e3, 1),
        "process_batch_ms": round(pb_ms, 3),
        "host_trim_ms": round(h_trim_ms, 3), "host_prior_ms": round(h_prior_ms, 3), "host_prior_how": prior_how,
        "host_outlier_stats_ms": round(h_out_ms, 3),
        "device_vs_host": {
            "trim_equal": [(int(s), int(e)) for s, e in zip(start.tolist(), end.tolist())] == [tuple(t) for t in h_trim],
            "prior_max_rel_where_ge_1e-30": rel,
            "keep_equal": all(np.array_equal(keep[b, :durs[b]].astype(bool), h_keep[b][0]) for b in range(B)),
        },
        "speed_bar": None,
        "note": "no speed bar is set; the host restatement timed in the same run is the comparison.  librosa parity of the trim is UNPINNED "
                "(librosa is not installed): the trim kernel is pinned against a float64 restatement of librosa 0.7.2 effects.trim only",
        "steps": a.steps, "warmup": a.warmup,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
