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

    python tools/bench_griffinlim.py [--steps 10] [--warmup 2] [--out profiles/griffinlim_bench.json]

With --momentum M the tool reports on fast Griffin-Lim instead (one JSON line of its own, nothing of the above is run): on the canonical
ragged batch of speech-like magnitudes (tests/griffinlim_restate.py speechlike_magnitude, a seeded start shared by both loops) the
per-iteration launch of the plain and of the momentum kernel (HIP events over back-to-back launches, and a torch.profiler kernel trace),
the whole call plain x 60 against momentum M x --iters (default 32), the spectral convergence || |STFT(x)| - mag || / || mag || of both,
the smallest iteration count at which momentum reaches the plain loop's convergence after 60, and with --device-phase the wall time of
a default angles=None call (host draw + copy) against a seed= call (phase drawn by the kernel).

    python tools/bench_griffinlim.py --momentum 0.99 --iters 32 --device-phase --out profiles/griffinlim_fast_bench.json

--quality (opt-in, both reports) adds the mel-cepstral distortion (ctts_amd.metrics, MFCC-style: the DCT of this project's log-mel, not
WORLD / SPTK mel-cepstra) of each Griffin-Lim output, its log-mel re-extracted by `TacotronSTFT`, against the log-mel of the magnitudes
it was given, frame by frame (align="none"); with --momentum also of the fast output against the plain one (`compare_wavs`), and the
sample-aligned waveform metrics of the fast output against the plain one (`waveform_metrics`: STOI, ESTOI, SI-SDR, multi-resolution
STFT distances; corpus means - two phase reconstructions of one magnitude, so SI-SDR is low by construction; the magnitudes are
synthetic, there is no recording to take them against).  Without the flag the output is unchanged."""
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
import ctts_amd  # noqa: E402,F401
from ctts_amd import audio, kernels as K  # noqa: E402
from ctts_amd.synthetic import make_batch  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
from griffinlim_restate import StockSTFT, seeded_angles, speechlike_magnitude  # noqa: E402

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


def mcd_vs_input(mag, frame_lens, sig):
    """mag [B,513,F] (what Griffin-Lim was given), frame_lens [B], sig [B, 256 (F - 1)] -> MCD dB (path_len-weighted) of the signal's
    re-extracted log-mel against log(clamp(mel_basis mag)), frame i against frame i"""
    from ctts_amd import metrics as M
    tac = audio.TacotronSTFT(NFFT, HOP, NFFT, 80, SR, 0, 8000).to(mag.device)
    mel_in = audio.dynamic_range_compression(torch.matmul(tac.mel_basis, mag)).contiguous()
    fl = torch.as_tensor(frame_lens, dtype=torch.int32).to(mag.device)
    mel, frames, _ = M.wav_features(sig, HOP * (fl - 1), tac)
    return round(M.summarize(M.compare_mels(mel_in, fl, mel, frames, align="none"))["mcd_db"].item(), 4)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def wall_ms(fn, steps, warmup):
    """median wall-clock ms of fn() with the device drained before and after: what a caller waits for, host work included"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def fast_report(a):
    dev = torch.device("cuda:0")
    stft = audio.STFT(NFFT, HOP, NFFT).to(dev)
    mom, n_fast = float(a.momentum), a.iters if a.iters is not None else 32
    coef = mom / (1.0 + mom)
    lens = [min(int(v), 1024) for v in make_batch(seed=1234)["mel_lens"]]
    B, Fmax = len(lens), max(lens)
    mag_h = np.zeros((B, 513, Fmax), dtype=np.float32)
    for b, F in enumerate(lens):
        mag_h[b, :, :F] = speechlike_magnitude(F, 100 + b)[0]
    mag = torch.from_numpy(mag_h).to(dev)
    ang = torch.from_numpy(seeded_angles(mag_h.shape, 22)).to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    samples = [HOP * (F - 1) for F in lens]

    def convergence(sig):
        """spectral convergence per utterance (its own frames only) and over the whole batch"""
        got, _ = stft.transform(sig, lens=samples)
        num = den = 0.0
        per = []
        for b, F in enumerate(lens):
            d = float((got[b, :, :F].double() - mag[b, :, :F].double()).pow(2).sum())
            m = float(mag[b, :, :F].double().pow(2).sum())
            per.append((d / m) ** 0.5)
            num, den = num + d, den + m
        return {"batch": round((num / den) ** 0.5, 5), "median": round(statistics.median(per), 5), "max": round(max(per), 5)}

    def run(n, momentum):
        return audio.griffin_lim(mag, stft, n, angles=ang, lens=lens_d, momentum=momentum)

    plain_ms, plain_out = timed(lambda: run(ITERS, 0.0), a.steps, a.warmup)
    fast_ms, fast_out = timed(lambda: run(n_fast, mom), a.steps, a.warmup)
    conv_plain, conv_fast = convergence(plain_out), convergence(fast_out)
    curve = {"plain": {}, "momentum": {}}
    match = None
    for n in range(1, ITERS + 1):
        c = convergence(run(n, mom))["batch"]
        if match is None and c <= conv_plain["batch"]:
            match = n
        if n in (8, 16, 24, 32, 48, 60):
            curve["momentum"][str(n)] = c
            curve["plain"][str(n)] = convergence(run(n, 0.0))["batch"]
    # the two launches alone: ITERS back-to-back launches on the same frame buffers
    ws = stft._workspace(mag, "magnitude")
    Y, magT = K.istft_frames(mag, ang, ws, lens_d, want_magT=True)
    Y2 = torch.empty_like(Y)
    state = K.griffinlim_state(B, Fmax, dev)
    K.griffinlim_iter_momentum(Y, magT, state, ws, Y2, coef, True, lens_d)      # fills the state: the timed launches read it

    def iters_plain():
        for _ in range(ITERS):
            K.griffinlim_iter(Y, magT, ws, Y2, lens_d)

    def iters_mom():
        for _ in range(ITERS):
            K.griffinlim_iter_momentum(Y, magT, state, ws, Y2, coef, False, lens_d)
    launch = {}
    for name, fn in (("plain", iters_plain), ("momentum", iters_mom)):
        loop_ms, _ = timed(fn, a.steps, a.warmup)
        k_us = kernel_us(fn, "gl_iter_kernel")
        launch[name] = {"iter_loop_us": round(loop_ms / ITERS * 1e3, 1), "iter_kernel_us": round(k_us, 1) if k_us else None}
    launch["momentum_over_plain_loop"] = round(launch["momentum"]["iter_loop_us"] / launch["plain"]["iter_loop_us"], 3)
    frames = sum(lens)
    res = {"tool": "tools/bench_griffinlim.py --momentum", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "steps": a.steps, "warmup": a.warmup, "momentum": mom, "B": B, "frames": frames, "max_frames": Fmax,
           "audio_s": round(sum(samples) / SR, 2), "input": "speechlike_magnitude(F_b, 100 + b), seeded_angles(seed 22)",
           "iter_launch": launch,
           "state_mb": round(state.numel() * 4 / 1e6, 1),
           "total": {"plain": {"iters": ITERS, "ms": round(plain_ms, 3), "spectral_convergence": conv_plain},
                     "momentum": {"iters": n_fast, "ms": round(fast_ms, 3), "spectral_convergence": conv_fast},
                     "speedup": round(plain_ms / fast_ms, 2)},
           "convergence_by_iterations": curve,
           "momentum_iters_to_reach_plain_60": match}
    if a.quality:
        from ctts_amd import metrics as M
        tac = audio.TacotronSTFT(NFFT, HOP, NFFT, 80, SR, 0, 8000).to(dev)
        sl = torch.tensor(samples, dtype=torch.int32, device=dev)
        r = M.summarize(M.compare_wavs(plain_out, sl, fast_out, sl, tac, align="none"))
        wm = M.summarize_waveform(M.waveform_metrics(plain_out, fast_out, sl, SR))
        res["quality"] = {"plain_mcd_db_vs_input_mel": mcd_vs_input(mag, lens, plain_out),
                          "momentum_vs_plain_waveform": {k: wm[k]["mean"] for k in ("stoi", "estoi", "si_sdr", "sc", "log_mag", "lsd_db")},
                          "momentum_mcd_db_vs_input_mel": mcd_vs_input(mag, lens, fast_out),
                          "momentum_vs_plain": {"mcd_db": round(r["mcd_db"].item(), 5), "lf0_rmse_cents": r["lf0_rmse_cents"].item(),
                                                "vuv_error": r["vuv_error"].item(), "n_voiced": int(r["n_voiced"].item())}}
    if a.device_phase:
        wsteps = max(1, min(a.steps, 5))
        host_ms = wall_ms(lambda: audio.griffin_lim(mag, stft, ITERS, lens=lens_d), wsteps, 1)
        seed_t = torch.tensor([7], dtype=torch.int64, device=dev)
        seed_ms = wall_ms(lambda: audio.griffin_lim(mag, stft, ITERS, lens=lens_d, seed=seed_t), wsteps, 1)
        both_ms = wall_ms(lambda: audio.griffin_lim(mag, stft, n_fast, lens=lens_d, seed=seed_t, momentum=mom), wsteps, 1)
        t0 = time.perf_counter()
        np.angle(np.exp(2j * np.pi * np.random.rand(B, 513, Fmax)))
        draw_ms = (time.perf_counter() - t0) * 1e3
        res["initial_phase_wall_ms"] = {"angles_none_host_draw_plain_60": round(host_ms, 2), "host_draw_alone": round(draw_ms, 2),
                                        "seed_plain_60": round(seed_ms, 3), f"seed_momentum_{n_fast}": round(both_ms, 3),
                                        "angle_tensor_mb": round(B * 513 * Fmax * 4 / 1e6, 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--momentum", type=float, default=None, help="report on fast Griffin-Lim with this momentum (e.g. 0.99) instead")
    ap.add_argument("--iters", type=int, default=None, help="with --momentum: iterations of the momentum loop (default 32; plain runs 60)")
    ap.add_argument("--device-phase", action="store_true", help="with --momentum: time an angles=None call against a seed= call")
    ap.add_argument("--quality", action="store_true", help="add the mel-cepstral distortion of the outputs (see the module docstring)")
    a = ap.parse_args()
    if a.momentum is None and (a.iters is not None or a.device_phase):
        ap.error("--iters and --device-phase belong to the --momentum report")
    if a.momentum is not None:
        return fast_report(a)
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
        if a.quality:
            res["shapes"][name]["quality"] = {"native_mcd_db_vs_input_mel": mcd_vs_input(mag, lens, nat)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
