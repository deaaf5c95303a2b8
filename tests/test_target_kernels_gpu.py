"""GPU: the kernels whose outputs are decisions or exact copies, against the models of tests/target_restate.py (pinned on the CPU, on
these very inputs, by tests/test_target_restate_cpu.py - which also shows that each plausible misreading of a header would fail here).

  ctts_mas (csrc/align.hip)                    hard alignment and durations: EXACT equality with the model, on all three code paths
                                               (mas_lds_kernel<1>, <2>, the global-memory mas_kernel) and across the switches between them
  ctts_cwt_pitch (csrc/pitch.hip)              against the float64 model; ids exact outside a stated band around the rounding edges
  ctts_conv_weight_repack, _conv_dgrad_weights exact equality with index arithmetic

Tolerance rule of the pitch chain (that of tests/test_pitch_features_gpu.py; no figure comes from the kernel): the largest error of f0
and of den (relative to 1 + |ref|) against float64 may be TWIN_X = 3 x the largest error of the float32 twin - the same model run on
float32 arrays - on the same input.  The ids must equal the float64 ids on every frame whose float64 bin coordinate lies farther from
a rounding edge (coord + 0.5 integral) than 3 x the twin's largest coordinate error; the frames nearer than that are left out of the id
comparison only, may differ by one bin at most, and hold at most 1 % of a case (asserted for the reference alone in the CPU module).
Every id of every case lies in [1, f0_bin - 1]: the ids index the pitch embedding.

Measured on the MI355X (`pytest -s` prints every pair), worst over the five call forms of each T, kernel (twin):
     T      f0 abs err           den rel err          twin coord err        excluded frames      ids differing on them
     2   1.13e-06 (7.74e-07)  8.14e-07 (5.61e-07)  1.0e-05 .. 3.5e-05   0                    0
     3   9.12e-07 (6.41e-07)  6.90e-07 (4.32e-07)  1.6e-05 .. 2.4e-05   0                    0
   255   1.65e-06 (1.00e-06)  1.15e-06 (6.57e-07)  7.0e-05 .. 1.2e-04   0                    0
   256   1.43e-06 (1.10e-06)  9.66e-07 (7.26e-07)  7.7e-05 .. 1.3e-04   1 of 888  (0.11 %)   0
   257   1.34e-06 (9.89e-07)  9.51e-07 (6.45e-07)  7.4e-05 .. 8.6e-05   0                    0
  1025   1.62e-06 (1.15e-06)  1.10e-06 (8.04e-07)  9.7e-05 .. 1.3e-04   2 of 3195 (0.06 %)   0
The kernel sits at 1.0 .. 1.9 x the twin, not below it: its mean and std are taken in double, but what dominates both is the rounding of
f0 itself (half an ulp of a value near 7 .. 11 is 2.4e-7 .. 4.8e-7) and the device's expf / log2f / powf, which are good to an ulp
where numpy's float32 functions are all but correctly rounded.  NaN cases: T2_constant f0 2.62e-07 (2.62e-07), den 1.47e-07 (2.14e-07);
T257_zero_spec_w40 f0 1.17e-06 (8.60e-07), den 8.25e-07 (6.19e-07).  The twin depends on the host's numpy (its SIMD float32 functions):
on another CPU these figures move in the last digits and a frame may enter or leave the excluded band.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctts_amd  # noqa: F401
from ctts_amd import _lib, kernels as K
from tests import target_restate as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                           # a copy: the shared inputs are read-only


def _np(t):
    return t.detach().cpu().numpy()


def _lens(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


# ====================================================================================================================== MAS
@functools.lru_cache(maxsize=None)
def _mas_ref(name):
    attn, in_lens, out_lens = R.mas_cases()[name]
    return R.mas_batch(attn, in_lens, out_lens)


def _check_mas(name):
    attn, in_lens, out_lens = R.mas_cases()[name]
    hard, dur = K.mas(_dev(attn), _lens(in_lens), _lens(out_lens))
    want_h, want_d = _mas_ref(name)
    h, d = _np(hard), _np(dur)
    assert h.dtype == np.float32 and d.dtype == np.float32 and h.shape == want_h.shape and d.shape == want_d.shape
    for b in range(h.shape[0]):
        assert np.array_equal(h[b], want_h[b]), f"{name}: utterance {b} (in {in_lens[b]}, out {out_lens[b]}) differs at {np.argwhere(h[b] != want_h[b])[:8].tolist()}"
        assert np.array_equal(d[b], want_d[b]), f"{name}: durations of utterance {b} differ at {np.flatnonzero(d[b] != want_d[b])[:8].tolist()}"
    return hard, dur


@pytest.mark.parametrize("Tk", R.MAS_SWITCH_TK)
def test_mas_path_switch_and_ballot_words(Tk):
    """Tk across the 64-column ballot words, 256 | 257 (one -> two columns per thread) and 512 | 513 (LDS -> global memory);
    ragged: full, in_len = Tk - 1, in_len = 1"""
    _check_mas(f"switch_tk{Tk}")


@pytest.mark.parametrize("Tq", (R.MAS_LDS_TQ_LAST, R.MAS_LDS_TQ_NEXT))
def test_mas_lds_size_switch(Tq):
    """Tk = 512: the largest Tq whose back-pointer bits fit the 60 KB of LDS, and the next one (derivation: tests/target_restate.py)"""
    _check_mas(f"lds_tq{Tq}")


def test_mas_prefetch_chunk_edges():
    _check_mas("chunk")


def test_mas_more_tokens_than_frames():
    """the path cannot reach column 0: the reference's extra opt[0, 0] = 1 is a second cell of row 0, and one more frame in dur"""
    for name in ("more_tokens", "more_tokens_2col"):
        hard, dur = _check_mas(name)
        _, in_lens, out_lens = R.mas_cases()[name]
        for b, (il, ol) in enumerate(zip(in_lens, out_lens)):
            assert il > ol and hard[b, 0, 0].item() == 1.0 and hard[b, 0].sum().item() == 2.0
            assert dur[b].sum().item() == ol + 1 and hard[b].sum().item() == ol + 1


def test_mas_lengths_zero_negative_and_beyond_the_padding():
    hard, dur = _check_mas("lengths")
    _, in_lens, out_lens = R.mas_cases()["lengths"]
    for b, (il, ol) in enumerate(zip(in_lens, out_lens)):
        if il <= 0 or ol <= 0:
            assert not hard[b].any() and not dur[b].any()
    assert dur[4].sum().item() == 11.0                                     # (100, 100) clamps to the padded 11 x 6


@pytest.mark.parametrize("name", ("uniform_tk8", "uniform_tk64", "onehot", "block"))
def test_mas_exact_ties_and_true_zeros(name):
    """uniform attention: every comparison is an exact float32 tie, the `>=` rule decides the whole path; one-hot / block: -inf cells"""
    _check_mas(name)


@pytest.mark.parametrize("name", ("diagonal", "softmax_130x37"))
def test_mas_realistic_maps_batch_independence_and_repeatability(name):
    hard, dur = _check_mas(name)
    attn, in_lens, out_lens = R.mas_cases()[name]
    a = _dev(attn)
    for b in range(attn.shape[0]):                                         # each utterance equals its own B = 1 call, bit for bit
        h1, d1 = K.mas(a[b:b + 1].contiguous(), _lens(in_lens[b:b + 1]), _lens(out_lens[b:b + 1]))
        assert torch.equal(h1[0], hard[b]) and torch.equal(d1[0], dur[b]), b
    h2, d2 = K.mas(a, _lens(in_lens), _lens(out_lens))
    assert torch.equal(h2, hard) and torch.equal(d2, dur)


@pytest.mark.parametrize("name", ("switch_tk65", "switch_tk513"))          # an LDS shape and a global-memory shape
def test_mas_raw_abi_writes_every_output_over_guard_cells(name):
    attn, in_lens, out_lens = R.mas_cases()[name]                          # ragged: the cells outside T1 x T2 must be WRITTEN as zeros
    B, Tq, Tk = attn.shape
    n, G = B * Tq * Tk, 64

    def guarded(m, dtype):
        t = torch.empty(m + G, dtype=dtype, device=DEV)
        if dtype == torch.uint8:
            t.fill_(0xA5)
            return t, t[m:].clone()
        t[:m] = float("nan")
        t[m::2] = 1e30
        t[m + 1::2] = float("nan")
        return t, t[m:].view(torch.int32).clone()
    opt, opt_guard = guarded(n, torch.float32)
    dur, dur_guard = guarded(B * Tk, torch.float32)
    back, back_guard = guarded(n, torch.uint8)
    a, il, ol = _dev(attn), _lens(in_lens), _lens(out_lens)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _lib.load().ctts_mas(a.data_ptr(), il.data_ptr(), ol.data_ptr(), opt.data_ptr(), dur.data_ptr(), back.data_ptr(), B, Tq, Tk, stream) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(opt[:n]).all() and torch.isfinite(dur[:B * Tk]).all(), "every cell of opt and dur is written"
    assert torch.equal(opt[n:].view(torch.int32), opt_guard) and torch.equal(dur[B * Tk:].view(torch.int32), dur_guard)
    assert torch.equal(back[n:], back_guard)
    want_h, want_d = _mas_ref(name)
    assert np.array_equal(_np(opt[:n]).reshape(B, Tq, Tk), want_h) and np.array_equal(_np(dur[:B * Tk]).reshape(B, Tk), want_d)


# ====================================================================================================================== cwt pitch
@functools.lru_cache(maxsize=None)
def _margin(name, T=None):
    cases = R.cwt_cases(T) if T is not None else R.cwt_nan_cases()
    return R.cwt_margin(next(c for c in cases if c["name"] == name))


def _cwt_call(args):
    kw = dict(eps=R.PITCH_EPS, mel_min=R.F0_MEL_MIN, mel_max=R.F0_MEL_MAX, f0_bin=R.F0_BIN, nscale=args["nscale"], width=args["width"])
    if "uv" in args:
        kw["uv"] = _dev(args["uv"])
    else:
        kw["uv_chan"] = args["uv_chan"]
    return K.cwt_pitch(_dev(args["spec"]), _dev(args["mean"]), _dev(args["std"]), args["std_scale"], **kw)


def _check_cwt(case, m):
    """-> (f0 error, den error) against float64; asserts the module's rules for one case"""
    name, args = case["name"], case["args"]
    f0_t, den_t, ids_t = _cwt_call(args)
    f0, den, ids = _np(f0_t), _np(den_t), _np(ids_t)
    B, width = args["spec"].shape[0], args["width"]
    assert f0.dtype == np.float32 and den.dtype == np.float32 and ids.dtype == np.int64
    assert f0.shape == den.shape == ids.shape == (B, width)
    assert ids.min() >= 1 and ids.max() <= R.F0_BIN - 1, f"{name}: ids outside the pitch embedding table: {ids.min()} .. {ids.max()}"
    ok = m["finite"]
    assert np.array_equal(np.isnan(f0), ~ok), f"{name}: f0 is NaN exactly where the model's is"
    assert np.array_equal(den == 0, m["unvoiced"]), f"{name}: den == 0 exactly where unvoiced"
    e_f0 = e_den = 0.0
    if ok.any():
        e_f0 = np.abs(f0.astype(np.float64) - m["f0"])[ok].max()
        e_den = (np.abs(den.astype(np.float64) - m["den"]) / (1.0 + np.abs(m["den"])))[ok].max()
    diff = np.abs(ids - m["ids"])
    print(f"{name}: f0 abs err {e_f0:.3e} (twin {m['twin_f0']:.3e}), den rel err {e_den:.3e} (twin {m['twin_den']:.3e}), twin coord err "
          f"{m['twin_coord']:.3e}, excluded {m['excluded'].sum()} / {m['excluded'].size} frames, ids differing on them {(diff[m['excluded']] > 0).sum()}")
    assert e_f0 <= R.TWIN_X * m["twin_f0"], name
    assert e_den <= R.TWIN_X * m["twin_den"], name
    assert m["excluded"].mean() <= R.CWT_EXCLUDED_CAP
    keep = ~m["excluded"]
    assert np.array_equal(ids[keep], m["ids"][keep]), f"{name}: wrong bin at {np.argwhere(keep & (diff > 0))[:8].tolist()}"
    assert diff.max() <= 1, name
    f0_b, den_b, ids_b = _cwt_call(args)                                   # repeatability: bit-identical
    assert torch.equal(f0_b.view(torch.int32), f0_t.view(torch.int32)) and torch.equal(den_b.view(torch.int32), den_t.view(torch.int32))
    assert torch.equal(ids_b, ids_t)
    return e_f0, e_den


@pytest.mark.parametrize("T", R.CWT_T)
def test_cwt_pitch_against_float64(T):
    """per T: dense spec + uv; ld_spec = 11 + uv_chan (inference); ld_spec = 11 + uv at width T + 1 (model.py's repeated-column launch);
    dense + uv at width T + 40 (the target launch); ld_spec = 11 + uv at width T + 40.  std_scale 1.0 and 0.8.  Utterance 0 is unvoiced
    throughout (den = 0, bin 1), utterance 1 clamps to f0_bin - 1, utterance 2 falls below 50 Hz (bin 1 through the scaled branch)."""
    worst = np.zeros(4)
    for case in R.cwt_cases(T):
        m = _margin(case["name"], T)
        e_f0, e_den = _check_cwt(case, m)
        worst = np.maximum(worst, [e_f0, m["twin_f0"], e_den, m["twin_den"]])
    print(f"T = {T}: worst f0 {worst[0]:.2e} (twin {worst[1]:.2e}), den {worst[2]:.2e} (twin {worst[3]:.2e})")


def test_cwt_pitch_nan_contours_stay_inside_the_embedding_table():
    """T = 1 (unbiased std of one sample) and constant contours (std = 0): f0 is NaN exactly where the model's is, and every id is a
    valid row of the pitch embedding"""
    for case in R.cwt_nan_cases():
        m = _margin(case["name"])
        assert not m["finite"].all()
        _check_cwt(case, m)


# ====================================================================================================================== repacks
@pytest.mark.parametrize("cout,cin,k", R.REPACK_SHAPES)
def test_conv_weight_repack_modes_are_exact(cout, cin, k):
    n = cout * cin * k
    src = R.distinct_integers(n, 7 * cout + 3 * cin + k)
    s = _dev(src)
    for mode in (0, 1, 2, 4):
        dst = torch.full((n,), float("nan"), device=DEV)
        out = K.conv_weight_repack(s, dst, cout, cin, k, mode)
        assert out is dst
        want = R.conv_weight_repack(src, cout, cin, k, mode)
        bad = np.flatnonzero(_np(dst) != want)
        assert bad.size == 0, f"mode {mode}: {bad.size} misplaced elements, first at {bad[:8].tolist()}"
    # mode 3 accumulates: one float32 add per element into what dst holds, and again on the second call
    dst0 = np.random.default_rng(n).standard_normal(n).astype(np.float32) * 1000.0
    dst = _dev(dst0)
    K.conv_weight_repack(s, dst, cout, cin, k, 3)
    once = R.conv_weight_repack(src, cout, cin, k, 3, dst0)
    assert np.array_equal(_np(dst).view(np.int32), once.view(np.int32))
    K.conv_weight_repack(s, dst, cout, cin, k, 3)
    assert np.array_equal(_np(dst).view(np.int32), R.conv_weight_repack(src, cout, cin, k, 3, once).view(np.int32))


def test_conv_dgrad_weights_across_the_launch_batch():
    """33 tasks of mixed shapes: one launch of 32 and one of 1, each through its own 32 x 32 tiles with ragged edges"""
    tasks = R.dgrad_tasks()
    outs = K.conv_dgrad_weights([(_dev(src), cout, cin, k) for src, cout, cin, k in tasks])
    assert len(outs) == len(tasks) == R.DGRAD_TASKS
    for t, (o, (src, cout, cin, k)) in enumerate(zip(outs, tasks)):
        assert o.shape == (cin, k * cout) and o.dtype == torch.float32
        assert np.array_equal(_np(o), R.conv_dgrad_weights(src, cout, cin, k)), (t, cout, cin, k)
    assert K.conv_dgrad_weights([]) == []
