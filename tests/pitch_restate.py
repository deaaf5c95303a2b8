"""Float64 numpy restatements of the pitch-feature kernels (csrc/pitchtrack.hip), and their float32 twins.

Every function takes `dtype`: np.float64 is the reference the GPU tests compare against; np.float32 is THE SAME CODE on float32 arrays
(numpy >= 2 keeps float32 through np.fft and through arithmetic with Python scalars) and gives the "what fp32 arithmetic alone costs"
number the GPU tolerances are derived from (3 x the twin's error), like tests/attention_restate.py and tests/loss_restate64.py.

  track_pitch        the tracker as specified in include/ctts.h (Boersma-style autocorrelation; a specified algorithm, not parselmouth)
  convert_continuous_f0 / cont_lf0 / norm_interp_f0 / norm_scale / inverse_cwt
                     utils/pitch_tools.py:39-66,152-190,212-217,267-272 restated; pinned against the live reference by
                     tests/golden/g19_pitch_chain.npz (tests/test_pitch_restate_cpu.py)
  cwt_mexican_hat    pycwt's published `cwt(signal, dt, dj, s0, J, MexicanHat())` - pycwt is not installed here, PARITY UNPINNED;
                     pinned instead by a closed form and by inverse_cwt reconstructing the contour
  f0_targets         the whole chain with the kernel's `valid` rule
"""
import math

import numpy as np

SR, HOP, FRAME, NFFT = 22050, 256, 1024, 2048
F0_MIN, F0_MAX, VOICING, SILENCE = 80.0, 750.0, 0.6, 0.03
CWT_DT, CWT_S0, CWT_J = 0.005, 0.01, 9

# ---- measured on the inputs of tests/test_pitch_restate_cpu.py with the float64 restatement ------------------
TRACKER_WORST_REL_ERR = 4.58e-4      # worst |f0 - true| / true over the voiced frames of the tones and the glide; the test asserts 2 x this
TRACKER_TONES_WORST_REL_ERR = 6.43e-3  # the same over the 15 stationary tones of gpu_tracker_cases() (every rate, hop and pitch range; the worst is
                                     # 110 Hz at 48 kHz, 2.3 periods per frame); the GPU test asserts 2 x this against the true frequency
DECISION_DELTA = 1.2e-6             # 4 x the largest |fp32 - fp64| candidate height on those inputs, the GPU test batches and gpu_tracker_cases()
                                     # (4 x 2.83e-7 = 1.13e-6, rounded up; the largest is the 110 Hz tone at 48 kHz)
INVERSE_CWT_MIN_CORR = 0.912         # lowest Pearson correlation of inverse_cwt(W) with the normalised contour over the fixture tracks


def hann_periodic(n=FRAME):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def window_autocorr_norm(nlag=512):
    """r_w(tau) / r_w(0) of the periodic hann window, float64"""
    w = hann_periodic()
    r = np.array([np.dot(w[:FRAME - t], w[t:]) for t in range(nlag)])
    return r / r[0]


def lag_range(sr=SR, f0_min=F0_MIN, f0_max=F0_MAX):
    return int(math.floor(sr / f0_max)), int(math.ceil(sr / f0_min))


def frame_candidates(x, dtype, sr=SR, f0_min=F0_MIN, f0_max=F0_MAX, use_octave_cost=True, _tabs={}):
    """one frame of 1024 raw samples -> (lags, heights, costs) of its candidates in ascending integer lag, or None for r(0) <= 0"""
    key = np.dtype(dtype).name
    if key not in _tabs:
        _tabs[key] = (hann_periodic().astype(dtype), window_autocorr_norm().astype(dtype))
    win, rwn = _tabs[key]
    lo, hi = lag_range(sr, f0_min, f0_max)
    x = np.asarray(x, dtype)
    xw = (x - x.mean(dtype=dtype)) * win
    X = np.fft.rfft(xw, NFFT)
    P = X.real * X.real + X.imag * X.imag
    r = np.fft.irfft(P, NFFT)[:512]
    assert r.dtype == np.dtype(dtype), "np.fft must keep the dtype (numpy >= 2)"
    r0 = r[0]
    if not (r0 > 0 and np.isfinite(r0)):
        return None
    rn = (r / r0) / rwn
    tau = np.arange(lo, hi + 1)
    a, b, c = rn[tau - 1], rn[tau], rn[tau + 1]
    m = (b > a) & (b >= c)
    tau, a, b, c = tau[m], a[m], b[m], c[m]
    den = (a - b) + (c - b)
    dl = dtype(0.5) * (a - c) / den
    lag = tau.astype(dtype) + dl
    h = b - dtype(0.25) * (a - c) * dl
    cost = h - dtype(0.01) * np.log2(dtype(f0_min) * lag / dtype(sr)) if use_octave_cost else h.copy()
    return lag, h, cost


def track_pitch(wav, lens=None, sr=SR, hop=HOP, f0_min=F0_MIN, f0_max=F0_MAX, voicing_threshold=VOICING, silence_threshold=SILENCE,
                dtype=np.float64, use_octave_cost=True, details=None, levels=None):
    """wav [B,N] -> (f0 [B,F], strength [B,F]); `details` (a list) receives (b, t, lags, heights, costs, winner index) per analysed frame
    that has a candidate, `levels` (a list) receives (b, t, frame peak, utterance peak) for the same frames"""
    wav = np.asarray(wav, dtype)
    B, N = wav.shape
    F = 1 + N // hop
    f0 = np.zeros((B, F), dtype)
    st = np.zeros((B, F), dtype)
    for b in range(B):
        n = N if lens is None else int(min(max(int(lens[b]), 0), N))
        peak = np.abs(wav[b, :n]).max() if n else dtype(0)
        for t in range(min(F, 1 + n // hop)):
            idx = t * hop - FRAME // 2 + np.arange(FRAME)
            x = np.where((idx >= 0) & (idx < n), wav[b, np.clip(idx, 0, N - 1)], dtype(0)).astype(dtype)
            cand = frame_candidates(x, dtype, sr, f0_min, f0_max, use_octave_cost)
            if cand is None or len(cand[0]) == 0:
                continue
            lag, h, cost = cand
            w = int(np.argmax(cost))                                   # first maximum = the smaller lag on a tie
            st[b, t] = h[w]
            if h[w] >= dtype(voicing_threshold) and np.abs(x).max() >= dtype(silence_threshold) * peak:
                f0[b, t] = dtype(sr) / lag[w]
            if details is not None:
                details.append((b, t, lag, h, cost, w))
            if levels is not None:
                levels.append((b, t, float(np.abs(x).max()), float(peak)))
    return f0, st


# ------------------------------------------------------------------------------------------------------------------ the target chain
def _interp_linear(x_new, xp, fp):
    """scipy interp1d(kind='linear') / np.interp inside the node range: slope * (x - x_lo) + y_lo with hi = searchsorted (left), clipped"""
    hi = np.clip(np.searchsorted(xp, x_new), 1, len(xp) - 1)
    lo = hi - 1
    slope = (fp[hi] - fp[lo]) / (xp[hi] - xp[lo]).astype(fp.dtype)
    return slope * (x_new - xp[lo]).astype(fp.dtype) + fp[lo]


def convert_continuous_f0(f0, dtype=np.float64):
    """utils/pitch_tools.py:152-183 - (uv, cont_f0); uv here has the REFERENCE function's polarity (1 = voiced)"""
    f0 = np.array(f0, dtype)
    uv = np.float32(f0 != 0)
    if (f0 == 0).all():
        return uv, f0
    start_f0, end_f0 = f0[f0 != 0][0], f0[f0 != 0][-1]
    start_idx = np.where(f0 == start_f0)[0][0]           # located by VALUE (:171-172)
    end_idx = np.where(f0 == end_f0)[0][-1]
    f0[:start_idx] = start_f0
    f0[end_idx:] = end_f0
    nz = np.where(f0 != 0)[0]
    if len(nz) == 1:                                     # a one-frame track: interp1d needs two nodes (the reference raises here)
        return uv, f0
    return uv, _interp_linear(np.arange(len(f0)), nz, f0[nz])


def cont_lf0(f0, dtype=np.float64):
    """get_cont_lf0 (:186-190)"""
    uv, c = convert_continuous_f0(f0, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        return uv, np.log(c)


def norm_interp_f0(f0, eps=1e-9, dtype=np.float64):
    """:39-66 with pitch_norm 'log', use_uv True -> (f0 target, uv) with uv = (f0 == 0)"""
    f0 = np.array(f0, dtype)
    uv = f0 == 0
    y = np.log2(f0 + dtype(eps))
    y[uv] = 0
    if uv.all():
        y[:] = 0
    elif uv.any():
        xp = np.where(~uv)[0]
        x = np.where(uv)[0]
        fp = y[~uv]
        if len(xp) == 1:
            y[uv] = fp[0]
        else:
            v = _interp_linear(x, xp, fp)
            v[x < xp[0]] = fp[0]
            v[x > xp[-1]] = fp[-1]
            y[uv] = v
    return y, uv


def cwt_scales():
    return CWT_S0 * 2.0 ** np.arange(CWT_J + 1)


def mexican_hat_ft(f):
    """pycwt MexicanHat = DOG(m = 2): psi_ft(f) = -(1j ** m) / sqrt(gamma(m + 0.5)) * f ** m * exp(-0.5 f ** 2), real for m = 2"""
    return f * f * np.exp(-0.5 * f * f) / type(f.flat[0])(math.sqrt(math.gamma(2.5)))


def cwt_mexican_hat(x, dtype=np.float64, wrong_norm=False):
    """real(pycwt.cwt(x, 0.005, 1, 0.01, 9, MexicanHat())[0]).T -> [n, 10]"""
    x = np.asarray(x, dtype)
    n = len(x)
    M = 1 << max(n - 1, 0).bit_length()                  # 2^ceil(log2 n)
    if M < 2:
        return np.zeros((n, CWT_J + 1), dtype)           # pycwt indexes ftfreqs[1]: a one-sample signal has no transform
    X = np.fft.fft(x, M)
    w = (2.0 * np.pi * np.fft.fftfreq(M, CWT_DT)).astype(dtype)
    out = np.zeros((n, CWT_J + 1), dtype)
    for j, s in enumerate(cwt_scales()):
        s = dtype(s)
        with np.errstate(invalid="ignore"):              # M = 2: w[1] is the Nyquist bin, negative - NaN, as in pycwt
            norm = np.sqrt(s * w[1] * dtype(M)) if not wrong_norm else np.sqrt(s)
        out[:, j] = np.fft.ifft(X * (norm * mexican_hat_ft(s * w)))[:n].real
    assert out.dtype == np.dtype(dtype)
    return out


def norm_scale(W):
    """:212-217"""
    mean, std = W.mean(0)[None, :], W.std(0)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (W - mean) / std, mean, std


def inverse_cwt(W, scales):
    """:267-272"""
    b = (np.arange(0, len(scales))[None, None, :] + 1 + 2.5) ** (-2.5)
    rec = (W * b).sum(-1)
    return (rec - rec.mean(-1, keepdims=True)) / rec.std(-1, keepdims=True)


def f0_targets(f0, frames, dtype=np.float64):
    """f0 [B,F], frames [B] -> dict(uv, cont_lf0, f0_mean, f0_std, cwt_spec, valid) with the kernel's rules: padding frames zero; valid = 0
    and all-zero rows without a voiced frame, for a constant contour (std == 0, decided as max == min) or a non-finite output"""
    f0 = np.asarray(f0, dtype)
    B, F = f0.shape
    out = dict(uv=np.zeros((B, F), dtype), cont_lf0=np.zeros((B, F), dtype), f0_mean=np.zeros(B, dtype), f0_std=np.zeros(B, dtype),
               cwt_spec=np.zeros((B, F, CWT_J + 1), dtype), valid=np.zeros(B, np.int32))
    for b in range(B):
        n = int(min(max(int(frames[b]), 0), F))
        if n == 0 or (f0[b, :n] == 0).all():
            continue
        _, lf = cont_lf0(f0[b, :n], dtype)
        if not np.isfinite(lf).all() or not lf.max() > lf.min():
            continue
        mean, std = np.mean(lf), np.std(lf)
        W = cwt_mexican_hat((lf - mean) / std, dtype)
        if not (np.isfinite(W).all() and np.isfinite(mean) and np.isfinite(std) and std > 0):
            continue
        out["uv"][b, :n] = f0[b, :n] == 0
        out["cont_lf0"][b, :n] = lf
        out["f0_mean"][b], out["f0_std"][b] = mean, std
        out["cwt_spec"][b, :n] = W
        out["valid"][b] = 1
    return out


def norm_interp_f0_batch(f0, frames, eps=1e-9, dtype=np.float64):
    f0 = np.asarray(f0, dtype)
    y, uv = np.zeros_like(f0), np.zeros_like(f0)
    for b in range(f0.shape[0]):
        n = int(min(max(int(frames[b]), 0), f0.shape[1]))
        if n:
            y[b, :n], u = norm_interp_f0(f0[b, :n], eps, dtype)
            uv[b, :n] = u
    return y, uv


# ------------------------------------------------------------------------------------------------------------------ test inputs
def harmonic_tone(freq_hz, n, sr=SR, phase=0.0):
    """fundamental + five harmonics with 1/k amplitudes, peak-normalised to 0.5; freq_hz: a scalar or the per-sample frequency [n]"""
    f = np.broadcast_to(np.asarray(freq_hz, np.float64), (n,))
    ph = 2.0 * np.pi * np.cumsum(f) / sr + phase
    x = sum(np.sin(k * ph) / k for k in range(1, 7))
    return 0.5 * x / np.abs(x).max()


TONES_HZ = (90.0, 110.0, 220.0, 440.0, 700.0)
GLIDE_HZ = (120.0, 240.0)
GROUND_TRUTH_N = 6144                                      # 25 frames per input


def ground_truth_inputs():
    """name -> (wav float64 [N], true F0 per frame [F] or None for 'must be unvoiced')"""
    n = GROUND_TRUTH_N
    F = 1 + n // HOP
    out = {}
    for f in TONES_HZ:
        out[f"tone{int(f)}"] = (harmonic_tone(f, n), np.full(F, f))
    fi = np.linspace(GLIDE_HZ[0], GLIDE_HZ[1], n)
    out["glide"] = (harmonic_tone(fi, n), fi[np.minimum(np.arange(F) * HOP, n - 1)])
    out["noise"] = (0.3 * np.clip(np.random.default_rng(7).standard_normal(n) / 3.0, -1, 1), None)
    out["silence"] = (np.zeros(n), None)
    return out


def full_window_frames(n, hop=HOP):
    """frames whose 1024-sample window lies wholly inside [0, n): where a stationary tone's true F0 is the tone's"""
    t = np.arange(1 + n // hop)
    return t[(t * hop - FRAME // 2 >= 0) & (t * hop + FRAME // 2 <= n)]


GPU_TRACK_N, GPU_TRACK_LENS = 6656, (6615, 5000, 1300)


def gpu_tracker_batch():
    """the GPU tracker test's ragged batch (float32 [3, 6656]): a glide, a tone whose second half is noise, a short tone; garbage past
    each length (it must not be read)"""
    rng = np.random.default_rng(11)
    w = 0.25 * rng.standard_normal((3, GPU_TRACK_N))       # what lies beyond lens
    n0, n1, n2 = GPU_TRACK_LENS
    w[0, :n0] = harmonic_tone(np.linspace(150.0, 260.0, n0), n0)
    w[1, :n1] = harmonic_tone(330.0, n1)
    w[1, n1 // 2:n1] = 0.3 * np.clip(rng.standard_normal(n1 - n1 // 2) / 3.0, -1, 1)
    w[2, :n2] = harmonic_tone(190.0, n2)
    return np.clip(w, -1, 1).astype(np.float32)


def gpu_silence_batch():
    """[2, 6656]: pure digital silence, and a tone"""
    w = np.zeros((2, GPU_TRACK_N), np.float32)
    w[1] = harmonic_tone(140.0, GPU_TRACK_N).astype(np.float32)
    return w


# ---- tracker inputs over the whole lag range, other rates / hops / pitch ranges and the two thresholds ------------------------------
# Every case: wav float32 [B, N <= 6144], lens (or None), the keyword arguments of track_pitch, and per utterance the true F0 of a
# stationary tone (None: not one).  tests/test_pitch_restate_cpu.py holds every case to the decision margins; the GPU test runs each as
# one launch.  Lag = sr / f0 falls in lane lag mod 64, register m = lag // 64 of pitch_track_kernel.
EDGE_TONES_HZ = (81.0, 84.0, 740.0)                         # winners at lags 270-272 and 261-263 (m = 4), 29.8 (lag_lo = 29, m = 0)
RAGGED_LENS = (6000, 100, 7000, -5, 3333)                   # no multiple of hop; shorter than half a frame; > N and < 0 clamp
PARAM_SETS = {
    "sr16k": dict(sr=16000, hop=200, f0_min=60.0, f0_max=400.0),     # lags 40..267
    "sr48k": dict(sr=48000, hop=512, f0_min=100.0, f0_max=1200.0),   # lags 40..480
    "f0min50": dict(f0_min=50.0),                                    # lag_hi = 441: registers m = 5, 6
}
SILENCE_LOW, VOICING_LOW = 0.01, 0.4                         # the non-default thresholds of the two threshold cases
SILENCE_STEP = 3000                                          # the sample at which the silence case's first utterance drops to 2 %
VOICING_NOISE_SEED = 3                                       # keeps every frame within the margins of the CPU test; to be replaced if it stops


def _garbage(rng, shape):
    return np.clip(0.25 * rng.standard_normal(shape), -1, 1)


def ragged_batch():
    """[5, 6144] with RAGGED_LENS and NaN-free garbage past each length: a rising glide, 100 samples of a tone, a falling glide whose
    length clamps to N, an utterance of clamped length 0, a tone with vibrato.  F = 25 is no multiple of a wave's four frames, so
    utterance boundaries fall inside waves, and B F = 125 is no multiple of a workgroup's 16."""
    n = GROUND_TRUTH_N
    rng = np.random.default_rng(23)
    w = _garbage(rng, (5, n))
    n0, n1, _, _, n4 = RAGGED_LENS
    w[0, :n0] = harmonic_tone(np.linspace(150.0, 260.0, n0), n0)
    w[1, :n1] = harmonic_tone(300.0, n)[:n1]
    w[2] = harmonic_tone(np.linspace(300.0, 200.0, n), n)
    w[4, :n4] = harmonic_tone(180.0 * (1.0 + 0.08 * np.sin(2.0 * np.pi * 9.0 * np.arange(n4) / SR)), n4)
    return w.astype(np.float32)


def _voicing_input(seed=VOICING_NOISE_SEED):
    """a 150 Hz tone in white noise of the tone's own power: the winner's height sits near 0.5"""
    n = GROUND_TRUTH_N
    x = harmonic_tone(150.0, n)
    noise = np.random.default_rng(seed).standard_normal(n) * np.sqrt(np.mean(x * x))
    return np.clip(0.6 * (x + noise), -1, 1)


def _silence_input():
    """[2, 6144]: a 200 Hz tone at peak 0.5 that drops to 2 % of it at SILENCE_STEP; a 260 Hz tone at peak 0.012 throughout, which is
    above the silence threshold of its own peak and below 0.03 x the first utterance's"""
    n = GROUND_TRUTH_N
    w = np.stack([harmonic_tone(200.0, n), 0.024 * harmonic_tone(260.0, n)])
    w[0, SILENCE_STEP:] *= 0.02
    return w


def gpu_tracker_cases():
    """name -> dict(wav, lens, params, truth)"""
    n = GROUND_TRUTH_N
    gt = ground_truth_inputs()
    c = {}

    def add(name, wav, truth, lens=None, **params):
        wav = np.ascontiguousarray(np.asarray(wav, np.float32))
        c[name] = dict(wav=wav, lens=lens, params=params, truth=list(truth))

    add("ground_truth", np.stack([w for w, _ in gt.values()]), [t[0] if t is not None and k.startswith("tone") else None for k, (_, t) in gt.items()])
    add("edges", np.stack([harmonic_tone(f, n) for f in EDGE_TONES_HZ] + [harmonic_tone(200.0, n) + 0.3]), EDGE_TONES_HZ + (200.0,))
    add("ragged", ragged_batch(), [None] * 5, lens=RAGGED_LENS)
    add("ragged_sr16k", ragged_batch(), [None] * 5, lens=RAGGED_LENS, **PARAM_SETS["sr16k"])       # the same samples read at 16 kHz
    p = PARAM_SETS["sr16k"]
    add("sr16k", np.stack([harmonic_tone(f, n, p["sr"]) for f in (70.0, 390.0)]), (70.0, 390.0), lens=(n, 4100), **p)
    p = PARAM_SETS["sr48k"]
    # 103 Hz (lag 466, m = 7) has 2.2 periods in a frame: tracked within the margins but too coarsely to be held to the true frequency
    add("sr48k", np.stack([harmonic_tone(f, n, p["sr"]) for f in (110.0, 1000.0, 103.0)]), (110.0, 1000.0, None), lens=(n, 5000, n), **p)
    add("f0min50", np.stack([harmonic_tone(f, n) for f in (55.0, 62.0)]), (55.0, 62.0), **PARAM_SETS["f0min50"])     # lags 401 (m = 6), 356 (m = 5)
    add("silence_default", _silence_input(), [None, None])
    add("silence_low", _silence_input(), [None, None], silence_threshold=SILENCE_LOW)
    add("voicing_default", _voicing_input()[None], [None])
    add("voicing_low", _voicing_input()[None], [None], voicing_threshold=VOICING_LOW)
    return c


def case_length(case, b):
    n = case["wav"].shape[1]
    return n if case["lens"] is None else int(min(max(case["lens"][b], 0), n))


# ---- target-chain inputs at the size edges of f0_targets_kernel: M = 2^ceil(log2 n) and CH = ceil(n / 256) per utterance ------------
CHAIN_EDGE_FRAMES = ((2, 3, 255, 256, 257, 512, 513), (2048, 2049))
CHAIN_LONG_N = 4096


def _contour(rng, n):
    t = np.arange(n)
    f = 170.0 + 50.0 * np.sin(t / 9.0) + 20.0 * np.cos(t / 2.3) + 2.0 * rng.standard_normal(n)
    f[(t % 23) < 5] = 0
    return f


def gpu_chain_edge_batches():
    """[(f0 float32 [B, F], frames)] for CHAIN_EDGE_FRAMES, F = the longest of each batch, garbage past each length"""
    rng = np.random.default_rng(17)
    out = []
    for frames in CHAIN_EDGE_FRAMES:
        F = max(frames)
        f0 = 100.0 + 200.0 * rng.random((len(frames), F))
        for b, n in enumerate(frames):
            f0[b, :n] = _contour(rng, n)
            if n == 2:
                f0[b, :2] = (150.5, 212.25)
            elif n == 3:
                f0[b, :3] = (180.0, 0.0, 210.5)
            else:
                f0[b, 40:70] = 0                                  # a gap across many chunks' summaries at CH = 1
                f0[b, n - 1] = 0 if b % 2 else 155.5              # the last frame of the utterance: unvoiced / voiced
        out.append((f0.astype(np.float32), frames))
    return out


def gpu_chain_long_runs():
    """f0 float32 [5, 4096], every utterance 4096 frames (CH = 16): a leading unvoiced run of 700 frames, an interior gap of 1500, a
    trailing run of 600, exactly two voiced frames (the first and the last), exactly one voiced frame"""
    n = CHAIN_LONG_N
    rng = np.random.default_rng(29)
    f0 = np.stack([_contour(rng, n) for _ in range(5)])
    f0[0, :700] = 0
    f0[1, 1000:2500] = 0
    f0[2, n - 600:] = 0
    f0[3] = 0; f0[3, 0] = 150.0; f0[3, n - 1] = 230.0
    f0[4] = 0; f0[4, 2000] = 175.0
    f0[0, 700] = 201.5; f0[1, 999] = 140.25; f0[1, 2500] = 260.5; f0[2, n - 601] = 188.0     # the runs' ends are voiced
    return f0.astype(np.float32), (n,) * 5


CHAIN_F, CHAIN_FRAMES = 64, (64, 37, 5, 1)


def gpu_chain_batch():
    """f0 [4, 64] float32 Hz for frames 64, 37, 5, 1 (M = 64, 64, 8, 1), garbage past each length"""
    rng = np.random.default_rng(5)
    f0 = (100.0 + 200.0 * rng.random((4, CHAIN_F))).astype(np.float32)
    t = np.arange(CHAIN_F)
    f0[0] = (180.0 + 40.0 * np.sin(t / 5.0) + 3.0 * rng.standard_normal(CHAIN_F)).astype(np.float32)
    f0[0, :3] = 0; f0[0, 20:29] = 0; f0[0, 40] = 0; f0[0, 60:] = 0
    f0[1, :37] = (120.0 + 1.5 * t[:37]).astype(np.float32)
    f0[1, 5:11] = 0; f0[1, 36] = 0
    f0[2, :5] = np.float32([0, 210.5, 0, 190.25, 0])
    f0[3, 0] = 150.0
    return f0


def gpu_chain_invalid_batch():
    """[3, 64], frames 64, 40, 64: all unvoiced; constant f0 with gaps (std == 0); a regular track"""
    f0 = np.zeros((3, CHAIN_F), np.float32)
    f0[1, :40] = 200.0
    f0[1, 3:9] = 0; f0[1, 39] = 0
    f0[2] = gpu_chain_batch()[0]
    return f0, (64, 40, 64)


FIXTURE_TRACKS = {
    # hand-made f0 tracks (Hz, 0 = unvoiced) of at most 64 frames for tests/golden/g19_pitch_chain.npz
    "lead_trail": [0, 0, 0, 180, 185, 0, 0, 190, 200, 210, 0, 0, 0, 205, 195, 0, 0],
    "repeat_first": [0, 150, 160, 150, 0, 0, 170, 180, 0, 175, 150, 0],
    "repeat_last": [140, 0, 0, 220, 230, 220, 0, 240, 220, 0, 0],
    "single": [0, 0, 0, 0, 123.5, 0, 0],
    "unvoiced": [0] * 9,
    "long": None,                                          # 64 frames, filled below
}
_t = np.arange(64)
_long = 200.0 + 50.0 * np.sin(_t / 7.0) + 10.0 * np.cos(_t / 2.0)
_long[(_t % 13) < 4] = 0
_long[:2] = 0
FIXTURE_TRACKS["long"] = [float(v) for v in _long]
FIXTURE_TRACKS = {k: np.asarray(v, np.float64) for k, v in FIXTURE_TRACKS.items()}
