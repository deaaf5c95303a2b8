"""Plain numpy models of the kernels whose outputs are decisions or exact copies, written from the kernel headers and include/ctts.h:

  mas                 ctts_mas (csrc/align.hip): monotonic alignment search, width 1 -> hard 0/1 alignment and durations.  Integer-exact:
                      the GPU comparison is array_equal.
  cwt_pitch           ctts_cwt_pitch (csrc/pitch.hip): inverse CWT -> normalisation -> f0 -> 2 ** f0 -> coarse bins.  Takes `dtype`:
                      np.float64 is the oracle, np.float32 is THE SAME CODE on float32 arrays (the twin: what fp32 arithmetic alone
                      costs, from which the GPU tolerances are derived like tests/pitch_restate.py).  Returns the UNROUNDED bin
                      coordinate next to the ids, so that a test can tell a frame near a rounding edge from a wrong bin.
  conv_weight_repack  ctts_conv_weight_repack modes 0 .. 4 and ctts_conv_dgrad_weights (csrc/elementwise.hip) as index arithmetic.
  conv_dgrad_weights

Each decision model takes `variant`: a deliberately WRONG reading of the header.  tests/test_target_restate_cpu.py asserts that every
variant differs from the right model on at least one input of the GPU module - an input set on which a wrong kernel could hide is
rejected there, without a GPU.

The inputs of tests/test_target_kernels_gpu.py are built here (mas_cases, cwt_cases, REPACK_SHAPES, dgrad_tasks) so that the CPU
module can pin the models on exactly those inputs."""
import functools
import math

import numpy as np

TWIN_X = 3.0                      # a GPU output may be this many times the float32 twin's largest error away from float64

# ====================================================================================================================== MAS
MAS_VARIANTS = ("strict_greater", "no_extra_one", "start_unclamped_column", "lengths_unclamped")


def mas(attn, in_len, out_len, variant=None):
    """One utterance.  attn [Tq, Tk] float32 soft attention -> (hard [Tq, Tk] float32 of 0 / 1, dur [Tk] float32).

    T1 = min(out_len, Tq) frames and T2 = min(in_len, Tk) tokens take part; everything outside T1 x T2 is zero, and everything is zero
    when either length is <= 0.  la[i, j] = float32(log(float64(attn[i, j]))).  Row 0 of the score is -inf except column 0; then, in
    float32, cur[j] = la[i, j] + (prev[j - 1] if j >= 1 and prev[j - 1] >= prev[j] else prev[j]), the first alternative recording
    "came from the left".  The path is walked back from (T1 - 1, T2 - 1), one cell per row; the reference's prev_ind[0, :] = 0 puts one
    more 1 at [0, 0], which is a second cell of row 0 whenever the path does not end there (more tokens than frames).  dur = column sums.

    Wrong variants (MAS_VARIANTS): `>` for `>=`; no extra [0, 0]; the walk started at column in_len - 1 (not clamped to the padded row,
    addressed in the flat [Tq * Tk] buffer like a kernel would) instead of T2 - 1; lengths not clamped at all (the rows and columns
    beyond the buffer read as attention 0 and are cropped from the result)."""
    assert variant is None or variant in MAS_VARIANTS, variant
    attn = np.asarray(attn, np.float32)
    Tq, Tk = attn.shape
    hard = np.zeros((Tq, Tk), np.float32)
    in_len, out_len = int(in_len), int(out_len)
    if in_len <= 0 or out_len <= 0:
        return hard, hard.sum(0)
    if variant == "lengths_unclamped":
        big = np.zeros((max(out_len, Tq), max(in_len, Tk)), np.float32)
        big[:Tq, :Tk] = attn
        h, _ = mas(big, in_len, out_len)
        hard = np.ascontiguousarray(h[:Tq, :Tk])
        return hard, hard.sum(0)
    T1, T2 = min(out_len, Tq), min(in_len, Tk)
    with np.errstate(divide="ignore"):
        la = np.log(attn[:T1, :T2].astype(np.float64)).astype(np.float32)
    ninf = np.float32(-np.inf)
    prev = np.full(T2, ninf, np.float32)
    prev[0] = la[0, 0]
    from_left = np.zeros((Tq, Tk), bool)                # flat-addressable, False outside T1 x T2 and in row 0
    for i in range(1, T1):
        left = np.concatenate([[ninf], prev[:-1]]).astype(np.float32)
        take = (left > prev) if variant == "strict_greater" else (left >= prev)
        take[0] = False
        with np.errstate(invalid="ignore"):             # -inf + inf cannot occur for probabilities <= 1; a NaN would only propagate
            prev = (la[i] + np.where(take, left, prev)).astype(np.float32)
        from_left[i, :T2] = take
    if variant == "start_unclamped_column":
        flat_h, flat_b = hard.reshape(-1), from_left.reshape(-1)
        cur = in_len - 1
        for i in range(T1 - 1, -1, -1):
            e = i * Tk + cur
            if e < flat_h.size:
                flat_h[e] = 1.0
            if i > 0 and e < flat_b.size and flat_b[e]:
                cur -= 1
    else:
        cur = T2 - 1
        for i in range(T1 - 1, -1, -1):
            hard[i, cur] = 1.0
            if i > 0 and from_left[i, cur]:
                cur -= 1
    if variant != "no_extra_one":
        hard[0, 0] = 1.0
    return hard, hard.sum(0)


def mas_batch(attn, in_lens, out_lens, variant=None):
    """attn [B, Tq, Tk] -> (hard [B, Tq, Tk], dur [B, Tk]) float32"""
    res = [mas(attn[b], in_lens[b], out_lens[b], variant) for b in range(attn.shape[0])]
    return np.stack([h for h, _ in res]), np.stack([d for _, d in res])


def _softmax_map(rng, B, Tq, Tk, sharp):
    x = rng.standard_normal((B, Tq, Tk)) * sharp
    x = np.exp(x - x.max(-1, keepdims=True))
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


def _diagonal_map(B, Tq, Tk, sigma=1.5):
    i, j = np.arange(Tq)[:, None], np.arange(Tk)[None, :]
    x = np.exp(-0.5 * ((j - i * (Tk - 1) / max(Tq - 1, 1)) / sigma) ** 2) + 1e-4
    x = (x / x.sum(-1, keepdims=True)).astype(np.float32)
    return np.repeat(x[None], B, 0).copy()


# ctts_mas takes the LDS kernels while Tq * (ceil(Tk / 64) * 8 + 2) + 12 * Tk <= 60 * 1024 = 61440 bytes (back-pointer bits [Tq][Tk / 64]
# of 8 bytes, two float rows + int durations = 12 Tk, a short per row) and Tk <= 512.  At Tk = 512 that is Tq * (8 * 8 + 2) + 12 * 512
# = 66 Tq + 6144 <= 61440, Tq <= 55296 / 66 = 837.8: Tq = 837 is the largest shape of the two-columns-per-thread LDS kernel, 838 the
# first that falls back to the global-memory kernel although Tk <= 512.
MAS_SWITCH_TK = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)     # ballot-word edges, 1 -> 2 columns per thread (256 | 257), LDS -> global (512 | 513)
MAS_LDS_TQ_LAST, MAS_LDS_TQ_NEXT = 837, 838
assert 66 * MAS_LDS_TQ_LAST + 12 * 512 <= 61440 < 66 * MAS_LDS_TQ_NEXT + 12 * 512
MAS_CHUNK_OUT_LENS = (1, 2, 8, 9, 10, 16, 17, 18)                   # rows 1 .. T1 - 1 in prefetch chunks of 8: 0, 1, 7, 8 | 9, 15 | 16, 17 rows


@functools.lru_cache(maxsize=None)
def mas_cases():
    """name -> (attn [B, Tq, Tk] float32, in_lens, out_lens).  Read-only: shared by the CPU pins and the GPU tests."""
    c = {}
    for Tk in MAS_SWITCH_TK:
        Tq = Tk + 9
        rng = np.random.default_rng(1000 + Tk)
        c[f"switch_tk{Tk}"] = (_softmax_map(rng, 3, Tq, Tk, 3.0), (Tk, Tk - 1, 1), (Tq, Tq - 3, Tq))
    for Tq in (MAS_LDS_TQ_LAST, MAS_LDS_TQ_NEXT):
        rng = np.random.default_rng(2000 + Tq)
        c[f"lds_tq{Tq}"] = (_softmax_map(rng, 3, Tq, 512, 2.0), (512, 511, 1), (Tq, Tq - 3, Tq))
    rng = np.random.default_rng(3)
    c["chunk"] = (_softmax_map(rng, 8, 18, 7, 3.0), (1, 2, 7, 7, 7, 7, 7, 7), MAS_CHUNK_OUT_LENS)
    c["more_tokens"] = (_softmax_map(rng, 2, 9, 8, 3.0), (7, 5), (3, 1))
    c["more_tokens_2col"] = (_softmax_map(rng, 1, 12, 300, 3.0), (300,), (5,))
    #                                            in 0  out 0  in > Tk  out > Tq  both   negative
    c["lengths"] = (_softmax_map(rng, 6, 11, 6, 3.0), (0, 4, 9, 6, 100, -3), (9, 0, 11, 20, 100, 8))
    for Tk, Tq in ((8, 20), (64, 70)):
        c[f"uniform_tk{Tk}"] = (np.full((2, Tq, Tk), 1.0 / Tk, np.float32), (Tk, Tk - 3), (Tq, Tq - 5))
    onehot = np.zeros((2, 40, 13), np.float32)
    onehot[:, np.arange(40), (np.arange(40) * 13) // 40] = 1.0
    c["onehot"] = (onehot, (13, 13), (40, 31))          # utterance 1 stops short of the last token: its corner cell is a true zero
    block = np.zeros((2, 40, 13), np.float32)
    for i in range(40):
        j = (i * 13) // 40
        block[:, i, max(j - 1, 0):j + 2] = 0.25         # exact ties inside the band, -inf outside it
    c["block"] = (block, (13, 9), (40, 40))
    c["diagonal"] = (_diagonal_map(3, 130, 37), (37, 30, 11), (130, 101, 64))
    c["softmax_130x37"] = (_softmax_map(np.random.default_rng(7), 3, 130, 37, 3.0), (37, 30, 11), (130, 101, 64))
    for a, _, _ in c.values():
        a.setflags(write=False)
    return c


# ====================================================================================================================== cwt pitch
F0_BIN = 256
F0_MEL_MIN = 1127.0 * math.log(1.0 + 50.0 / 700.0)         # include/ctts.h: mel_min / mel_max = 1127 ln(1 + f / 700) at 50 / 1100 Hz
F0_MEL_MAX = 1127.0 * math.log(1.0 + 1100.0 / 700.0)
PITCH_EPS = 1e-6
CWT_VARIANTS = ("std_over_width", "biased_std", "uv_indexed_at_T", "std_scale_ignored")


def cwt_pitch(spec, mean, std, std_scale, uv=None, uv_chan=-1, nscale=10, width=None, eps=PITCH_EPS, mel_min=F0_MEL_MIN,
              mel_max=F0_MEL_MAX, f0_bin=F0_BIN, dtype=np.float64, variant=None):
    """spec [B, T, ld >= nscale], mean / std [B] -> (f0 [B, width], den [B, width], coord [B, width], ids [B, width] int64), per utterance
         rec[t] = sum_{j < nscale} spec[t, j] * (j + 3.5) ** -2.5 (left to right);  rec = (rec - mean_t rec) / std_t rec, the std unbiased
         and both over ALL T columns;  columns T .. width - 1 repeat column T - 1;
         f0 = log2(exp(rec * std * std_scale + mean) + eps);   den = 0 where unvoiced else 2 ** f0;
         mel = 1127 ln(1 + den / 700);  coord = (mel - mel_min) * (f0_bin - 2) / (mel_max - mel_min) + 1 where mel > 0 else mel, clamped to
         [1, f0_bin - 1];  ids = floor(coord + 0.5).
    unvoiced = uv[b, t] > 0 (uv [B, width]) or, without uv, spec[b, t, uv_chan] > 0.  A NaN contour (T = 1, std = 0) keeps f0 = NaN;
    the clamp is C's fmax / fmin, which return the other operand for a NaN, so such a frame has coord 1 and id 1: inside the table.

    Wrong variants (CWT_VARIANTS): mean / std over the `width` repeated columns; biased std; uv read with row stride T instead of
    width; std_scale ignored."""
    assert variant is None or variant in CWT_VARIANTS, variant
    f = np.dtype(dtype).type
    spec = np.asarray(spec, dtype)
    B, T, ld = spec.shape
    width = T if width is None else int(width)
    assert width >= T and ld >= nscale
    mean, std = np.asarray(mean, dtype)[:, None], np.asarray(std, dtype)[:, None]
    taps = (np.arange(nscale).astype(dtype) + f(3.5)) ** f(-2.5)
    rec = np.zeros((B, T), dtype)
    for j in range(nscale):
        rec = rec + spec[:, :, j] * taps[j]
    col = np.minimum(np.arange(width), T - 1)
    stat = rec[:, col] if variant == "std_over_width" else rec
    n = stat.shape[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = stat.sum(1, keepdims=True) / f(n)
        var = ((stat - mu) ** 2).sum(1, keepdims=True) / f(n if variant == "biased_std" else n - 1)       # T = 1: 0 / 0 = NaN
        recn = (rec[:, col] - mu) / np.sqrt(var)                                                            # std = 0: 0 / 0 = NaN
        sd = std if variant == "std_scale_ignored" else std * f(std_scale)
        f0 = np.log2(np.exp(recn * sd + mean) + f(eps))
        if uv is not None:
            uv = np.asarray(uv)
            assert uv.shape == (B, width)
            if variant == "uv_indexed_at_T":
                unvoiced = uv.reshape(-1)[np.arange(B)[:, None] * T + np.arange(width)[None, :]] > 0
            else:
                unvoiced = uv > 0
        else:
            assert 0 <= uv_chan < ld and width == T
            unvoiced = spec[:, :, uv_chan] > 0
        den = np.where(unvoiced, f(0), f(2) ** f0)
        mel = f(1127) * np.log(f(1) + den / f(700))
        scaled = (mel - f(mel_min)) * f(f0_bin - 2) / (f(mel_max) - f(mel_min)) + f(1)
        coord = np.where(mel > 0, scaled, mel)
        coord = np.fmin(np.fmax(coord, f(1)), f(f0_bin - 1))
    ids = np.floor(coord + f(0.5)).astype(np.int64)
    assert f0.dtype == den.dtype == coord.dtype == np.dtype(dtype), "the arithmetic must stay in dtype"
    return f0, den, coord, ids


def cwt_margin(case):
    """-> dict: the float64 oracle (f0, den, coord, ids, unvoiced), the twin's largest errors on this input and the frames excluded
    from the id comparison: those whose float64 coord + 0.5 lies within TWIN_X x the twin's largest coordinate error of an integer."""
    r64 = cwt_pitch(dtype=np.float64, **case["args"])
    r32 = cwt_pitch(dtype=np.float32, **case["args"])
    f0, den, coord, ids = r64
    ok = np.isfinite(f0)
    assert np.array_equal(ok, np.isfinite(r32[0]))

    def worst(e):
        e = e[ok]
        return float(e.max()) if e.size else 0.0
    twin_f0 = worst(np.abs(r32[0].astype(np.float64) - f0))
    twin_den = worst(np.abs(r32[1].astype(np.float64) - den) / (1.0 + np.abs(den)))
    twin_coord = worst(np.abs(r32[2].astype(np.float64) - coord))
    x = coord + 0.5
    excluded = np.abs(x - np.round(x)) <= TWIN_X * twin_coord
    return dict(f0=f0, den=den, coord=coord, ids=ids, finite=ok, twin_ids=r32[3], twin_f0=twin_f0, twin_den=twin_den, twin_coord=twin_coord,
                excluded=excluded, unvoiced=den == 0)


CWT_T = (2, 3, 255, 256, 257, 1025)
CWT_FORMS = ("dense_uv", "uvchan", "ld11_uv_w1", "dense_uv_w40", "ld11_uv_w40")
CWT_EXCLUDED_CAP = 0.01
# The seeds (100 T + form index) are ones for which the float64 reference alone keeps the excluded share of every case within
# CWT_EXCLUDED_CAP (tests/test_target_restate_cpu.py::test_cwt_excluded_share_of_the_reference_alone); at T = 2, 3 that means no
# excluded frame at all.


def _cwt_case(T, form, seed):
    rng = np.random.default_rng(seed)
    B = 3
    ld = 10 if form.startswith("dense") else 11
    width = T + {"dense_uv": 0, "uvchan": 0, "ld11_uv_w1": 1, "dense_uv_w40": 40, "ld11_uv_w40": 40}[form]
    spec = (rng.standard_normal((B, T, ld)) * 0.6).astype(np.float32)
    mean = np.array([5.0, 7.3, 4.6], np.float32) + (rng.standard_normal(B) * 0.05).astype(np.float32)
    std = np.array([0.3, 0.3, 0.5], np.float32)           # utterance 1 reaches above 1100 Hz (bin f0_bin - 1), utterance 2 below 50 Hz (bin 1)
    args = dict(spec=spec, mean=mean, std=std, std_scale=0.8 if form in ("uvchan", "ld11_uv_w1") else 1.0, nscale=10, width=width)
    # Voicing.  Utterance 0 is unvoiced on every frame.  The tolerance of den is a SAMPLE maximum of the twin's error over the voiced
    # frames, and a maximum over two or three frames says little about the float32 error scale: at T <= 3 the other utterances are
    # voiced on every frame (as many samples as the shape allows); at the larger T on frame 0 and on about 70 % (50 %) of the rest.
    voiced = np.s_[1:, :] if T <= 3 else np.s_[1:, 0]
    if form == "uvchan":
        spec[0, :, 10] = 1.0
        spec[voiced + (10,)] = -1.0
        args.update(uv_chan=10)
    else:
        if ld == 11:                                        # model.py: the predictor's uv logit, last column repeated up to the width
            spec[0, :, 10] = 1.0
            spec[voiced + (10,)] = -1.0
            uv = (spec[:, :, 10] > 0).astype(np.float32)
            uv = np.concatenate([uv] + [uv[:, -1:]] * (width - T), 1)
        else:
            uv = (rng.random((B, width)) < 0.3).astype(np.float32)
            uv[0] = 1.0
            uv[voiced] = 0.0
        args.update(uv=np.ascontiguousarray(uv))
    for v in args.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dict(name=f"T{T}_{form}", args=args)


@functools.lru_cache(maxsize=None)
def cwt_cases(T):
    return tuple(_cwt_case(T, form, 100 * T + i) for i, form in enumerate(CWT_FORMS))


@functools.lru_cache(maxsize=None)
def cwt_nan_cases():
    """T = 1 (unbiased std of one sample) and constant contours (std = 0): f0 is NaN.  The constant contours are exact in every
    precision: T = 2 sums two equal values, and the all-zero spectrogram is 0 at any T."""
    rng = np.random.default_rng(11)
    mean, std = np.array([5.0, 5.2, 4.8], np.float32), np.array([0.3, 0.2, 0.4], np.float32)
    one = (rng.standard_normal((3, 1, 11)) * 0.6).astype(np.float32)
    two = np.repeat((rng.standard_normal((3, 1, 11)) * 0.6).astype(np.float32), 2, 1)
    two[1, 1] += 0.25                                       # utterance 1 is a regular two-frame contour,
    two[1, :, 10] = -1.0                                    # voiced
    zero = np.zeros((3, 257, 10), np.float32)
    zero[2] = (rng.standard_normal((257, 10)) * 0.6).astype(np.float32)
    uv = (rng.random((3, 297)) < 0.3).astype(np.float32)
    return (dict(name="T1_uvchan", args=dict(spec=one, mean=mean, std=std, std_scale=1.0, uv_chan=10, nscale=10, width=1)),
            dict(name="T1_uv_w5", args=dict(spec=one, mean=mean, std=std, std_scale=1.0, nscale=10, width=5,
                                            uv=np.array([[1, 0, 0, 1, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], np.float32))),
            dict(name="T2_constant", args=dict(spec=two, mean=mean, std=std, std_scale=0.8, uv_chan=10, nscale=10, width=2)),
            dict(name="T257_zero_spec_w40", args=dict(spec=zero, mean=mean, std=std, std_scale=1.0, nscale=10, width=297, uv=uv)))


# ====================================================================================================================== repacks
REPACK_SHAPES = ((1, 1, 1), (33, 31, 3), (64, 32, 1), (5, 70, 9), (512, 512, 9))     # the last: 2.4 M elements > 4096 blocks x 256 threads


def conv_weight_repack(src, cout, cin, k, mode, dst=None):
    """include/ctts.h ctts_conv_weight_repack on flat arrays, one output element at a time as index arithmetic:
         mode 0  dst[co][kk][ci] = src[co][ci][kk]           mode 1  dst[ci][kk][co] = src[co][ci][k - 1 - kk]
         mode 2  dst[co][ci][kk] = src[co][kk][ci]           mode 3  dst[co][ci][kk] += src[co][kk][ci]  (one float32 add)
         mode 4  dst[ci][kk][co] = src[co][k - 1 - kk][ci]"""
    src = np.asarray(src).reshape(-1)
    e = np.arange(cout * cin * k, dtype=np.int64)
    if mode == 0:
        ci, kk, co = e % cin, (e // cin) % k, e // (cin * k)
        out = src[(co * cin + ci) * k + kk]
    elif mode == 1:
        co, kk, ci = e % cout, (e // cout) % k, e // (cout * k)
        out = src[(co * cin + ci) * k + (k - 1 - kk)]
    elif mode == 4:
        co, kk, ci = e % cout, (e // cout) % k, e // (cout * k)
        out = src[(co * k + (k - 1 - kk)) * cin + ci]
    elif mode in (2, 3):
        kk, ci, co = e % k, (e // k) % cin, e // (k * cin)
        out = src[(co * k + kk) * cin + ci]
        if mode == 3:
            out = (np.asarray(dst, np.float32).reshape(-1) + out.astype(np.float32)).astype(np.float32)
    else:
        raise ValueError(mode)
    return out


def conv_dgrad_weights(src, cout, cin, k):
    """ctts_conv_dgrad_weights, one task: dst[ci][kk][co] = src[co][k - 1 - kk][ci] -> [cin, k * cout]"""
    return conv_weight_repack(src, cout, cin, k, 4).reshape(cin, k * cout)


def distinct_integers(n, seed):
    """n distinct integers below 2 ** 24 (exact in float32) in a scrambled order: any misplaced element shows"""
    assert n < 1 << 24
    return np.random.default_rng(seed).permutation(n).astype(np.float32)


DGRAD_SHAPES = ((33, 31, 3), (1, 1, 1), (32, 32, 5), (70, 5, 9), (64, 32, 1), (5, 70, 9), (31, 33, 2))
DGRAD_TASKS = 33                                            # one more than the 32 tasks of a launch


def dgrad_tasks():
    """-> list of (src [cout, k * cin] float32, cout, cin, k): DGRAD_TASKS tasks cycling through DGRAD_SHAPES"""
    out = []
    for t in range(DGRAD_TASKS):
        cout, cin, k = DGRAD_SHAPES[t % len(DGRAD_SHAPES)]
        out.append((distinct_integers(cout * cin * k, 500 + t).reshape(cout, k * cin), cout, cin, k))
    return out
