"""GPU: the vocoder layer kernels over the whole contract their entry points accept - vconv_kernel (csrc/vocoder.hip), vconv_h_kernel
(csrc/vocoder_h.hip), the shared geometry, epilogue and vpost_kernel (csrc/vocoder_common.h) - against the float64 layer model
tests/vocoder_layer_restate.py, in all three arithmetics: "split" (bf16_split = 1), "fp32" (bf16_split = 0) and "fp16" (vocoder_conv_h).
The feature tests (test_vocoder_gpu.py, _half_gpu.py, _ragged_gpu.py) visit V1's geometries only; here are the others:

  a  ConvTranspose1d over M.KU (one tap .. 65 taps, row_off 0 / 1 / 2, mextra 0 / 1, u = 1), N = u Cout below 32, off a multiple of 32 and
     on the 32-, 64- and 128-wide column tiles, T on both sides of the 128-row tile: integer operands, bit-exact
  b  the same geometries ragged: NaN beyond every length, a sentinel in `out`, each utterance bit-equal to its own B = 1 call
  c  Conv1d over M.KD (five of them with the full 64-row halo) at channel counts from 1 to 130, T below and above the padding, and the
     strided / channel-first / misaligned input forms bit-equal to the contiguous one
  d  the 16 on / off combinations of bias, R, alpha, beta (NaN in `out` when beta == 0)
  e  random operands against float64 within the rules test_vocoder_gpu.py and test_vocoder_half_gpu.py state
  f  what vc_geometry refuses raises before any launch, and Generator refuses the same configs
  g  conv_post directly: fp32, ragged and fp16 input, C and T around the 32-channel chunk and the 256-row tile
  h  whole generators that are not V1: the published V2 (upsample_initial_channel = 128) and an "odd" config (k = 3u and k = u
     upsamplers, channels 24 / 12 / 6, two ResBlocks per stage), dense and ragged

Integer operands follow test_vocoder_half_gpu.py's integer_case; the premise of "exact in any order" (sum of magnitudes <= 2048, the
fp16 integer range, which is below fp32's 2^24) is asserted in every case.

Bars.  e: fp32 err <= 16 ULP max|ref| max(1, sqrt(K)), split err <= 1.25 fp32 err + ULP max|ref| (K = taps x Cin, ULP = 2^-23); fp16
per element 2^-11 |ref| + K 2^-24 mag + 2^-24.  g: |out - tanh64| <= (k C + 2) 2^-24 mag (fp32 accumulation in any order, the leaky_relu
product and the bias add; tanh is 1-Lipschitz) + 3 x the largest error of the float32 twin - torch.tanh in float32 on the CPU of the
float32-rounded pre-activation - over the cases of the test.  h: fp32 / split max err <= 2 x the float32 CPU restatement's on the same
input; fp16 as test_v1_size_fp16_vs_fp64_restatement (rms <= 1.25 x, max <= 2 x the CPU emulation of the fp16 contract).

Measured on the MI355X (pytest -s prints every figure):
  a - d  every case bit-exact in the three arithmetics; nothing stored beyond an end, no NaN
  e  fp32 err 2.8e-7 .. 4.4e-6, at most 0.014 of its bar (k=1 36->130: 9.1e-7 of 6.8e-5); split err 3.4e-7 .. 3.9e-6, at most 0.76 of its
     bar (k=65 33->31 T=37: 1.95e-6 of 2.55e-6; k=12 u=4 40->24 T=129: 1.57e-6 of 2.20e-6); fp16 max err 1.5e-3 .. 2.2e-3, largest
     err / bound 0.42 (k=130 u=2 40->24) .. 0.984 (k=1 36->130): the stored value's own rounding is the whole of it at small K
  g  kernel max err (largest err / bar) k=1 8.5e-7 (0.23), k=3 1.5e-6 (0.26), k=7 1.8e-6 (0.14), k=31 3.0e-6 (0.06); float32 twin max err
     5.2e-8 .. 5.3e-8 in every family (allowance 1.6e-7); integer pre-activations: kernel 4.0e-8, twin 2.5e-8
  h  native err / float32 CPU restatement err: V2 split 6.5e-7 / 6.7e-7, V2 fp32 9.2e-7 / 6.7e-7, odd split 4.5e-7 / 3.2e-7, odd fp32
     4.3e-7 / 3.2e-7 (bar: 2 x); fp16 rms, max (emulation, larger order): V2 2.39e-4, 1.11e-3 (2.44e-4, 1.12e-3), odd 2.10e-4, 7.09e-4
     (2.13e-4, 8.25e-4)
No kernel, geometry, packer or Generator change was needed: the 86 tests passed on the code as it stood.
"""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctts_amd  # noqa: E402,F401
from ctts_amd import _lib  # noqa: E402
from ctts_amd import kernels as K  # noqa: E402
from ctts_amd.vocoder import AttrDict, Generator  # noqa: E402
import hifigan_restate as R  # noqa: E402
import test_vocoder_half_gpu as H  # noqa: E402      (integer operands, the fp16 bound and the fp16 generator rule, as that file states them)
import vocoder_layer_restate as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ARITHS = ("split", "fp32", "fp16")
ULP = 2.0 ** -23
NAN = float("nan")

# (k, u) -> the two (Cin, Cout) pairs it runs at; N = u Cout in the comment
UP_CH = {(2, 2): [(32, 32), (20, 12)],          # 64, 24
         (3, 3): [(16, 8), (64, 48)],           # 24, 144
         (8, 8): [(32, 32), (16, 8)],           # 256, 64
         (1, 1): [(20, 12), (40, 24)],          # 12, 24
         (3, 1): [(32, 32), (64, 48)],          # 32, 48
         (5, 1): [(16, 8), (40, 24)],           # 8, 24
         (4, 2): [(32, 32), (20, 12)],          # 64, 24
         (16, 8): [(64, 48), (16, 8)],          # 384, 64
         (6, 2): [(40, 24), (32, 32)],          # 48, 64
         (12, 4): [(32, 32), (20, 12)],         # 128, 48
         (9, 3): [(16, 8), (40, 24)],           # 24, 72
         (8, 2): [(64, 48), (20, 12)],          # 96, 24
         (16, 4): [(32, 32), (40, 24)],         # 128, 96
         (10, 2): [(16, 8), (64, 48)],          # 16, 96
         (15, 3): [(20, 12), (32, 32)],         # 36, 96
         (24, 4): [(40, 24), (16, 8)],          # 96, 32
         (130, 2): [(32, 32), (20, 12)]}        # 64, 24
UP_TS = [(1, 37, 127, 129), (2, 128, 300)]      # the T values of the first and of the second pair: Mrows = T + mextra on, before and past 128
CONV_CH = [(1, 1), (3, 5), (8, 8), (16, 8), (20, 36), (33, 31), (80, 100), (36, 130)]
CONV_TS = [1, 2, 63, 128, 129, 200]


def test_case_tables_reach_what_they_are_there_for():
    assert list(UP_CH) == M.KU
    ns = [u * cout for (k, u), pairs in UP_CH.items() for _, cout in pairs]
    tiles = {128 if n % 128 == 0 else (64 if n % 64 == 0 else 32) for n in ns}
    assert tiles == {32, 64, 128} and any(n < 32 for n in ns) and any(n > 32 and n % 32 for n in ns)
    assert {p for pairs in UP_CH.values() for p in pairs} == {(32, 32), (16, 8), (20, 12), (40, 24), (64, 48)}
    for k, u in M.KU:
        mextra = M.geometry(100, k, 1, u)["mextra"]
        assert any(T + mextra in (127, 128, 129) for ts in UP_TS for T in ts)
    for k, d in M.KD:                        # T not above the padding and T above it (k = 1 has no padding)
        ts = {T for i in range(len(CONV_CH)) for T in _conv_ts(i, k)}
        pad = d * (k - 1) // 2
        assert ts == set(CONV_TS) and any(T > pad for T in ts) and (pad == 0 or any(T <= pad for T in ts))


def _conv_ts(i, k):
    return CONV_TS[(i + k) % 6], CONV_TS[(i + k + 3) % 6]


# ---- one layer call in an arithmetic -------------------------------------------------------------------------------------------------
def _cin_cout(w, u):
    return (w.shape[0], w.shape[1]) if u else (w.shape[1], w.shape[0])


def _act(arith, t):
    """a float32 activation tensor in the arithmetic's own type (fp16 of small integers is exact)"""
    return t.half() if arith == "fp16" and t is not None else t


def run_layer(arith, x, w, dil=1, u=0, slope=None, bias=None, R_=None, out=None, alpha=1.0, beta=0.0, lens=None, len_mul=1):
    """x as the caller made it (dtype and strides); w the fp32 master weight; R_ / out float32 tensors, converted (and `out` cloned)
    here -> the kernel's result as float64"""
    cin, cout = _cin_cout(w, u)
    kw = dict(transposed_u=u, slope=slope, bias=bias, R=_act(arith, R_), out=None if out is None else _act(arith, out.clone()),
              alpha=alpha, beta=beta, lens=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV), len_mul=len_mul)
    if arith == "fp16":
        res = K.vocoder_conv_h(x, K.vocoder_pack_weight_h(w, u), cin, cout, w.shape[2], dil, **kw)
        assert res.dtype == torch.float16
    else:
        split = 1 if arith == "split" else 0
        wp, pl = K.vocoder_pack_weight(w, u, planes=split)
        res = K.vocoder_conv(x, wp, pl, cin, cout, w.shape[2], dil, bf16_split=split, **kw)
    return res.double()


def model(arith, x, w, *a, **kw):
    return M.conv_layer(x, w.half() if arith == "fp16" else w, *a, half=arith == "fp16", **kw)


def int_operands(B, T, cin, cout, k, u, g):
    """integer_case's operands (test_vocoder_half_gpu.py): x in {-4, -2, 0, 1, 2, 3} (slope 0.5 -> integers, |a| <= 3), sparse weights in
    {-2, 0, 2}, even bias and R, any integer in `old`: with alpha in {0.5, 1} and beta in {0, 2} every term is an integer"""
    x = torch.tensor([-4.0, -2.0, 0.0, 1.0, 2.0, 3.0])[torch.randint(0, 6, (B, T, cin), generator=g)]
    w = H.sparse_even_weight((cin, cout, k) if u else (cout, cin, k), cin * (k // u if u else k), g)
    Tout = T * u if u else T
    bias = (torch.randint(-2, 3, (cout,), generator=g) * 2).float()
    Rr = (torch.randint(-2, 3, (B, Tout, cout), generator=g) * 2).float()
    old = torch.randint(-4, 5, (B, Tout, cout), generator=g).float()
    return tuple(t.to(DEV) for t in (x, w, bias, Rr, old))


def assert_premise(ref, mag, stored=None):
    """every partial sum is bounded by the sum of magnitudes: integers of magnitude <= 2048 are exact in fp16, and 2048 < 2^24 in fp32 -
    in any summation order"""
    if stored is not None:
        ref, mag = ref[stored], mag[stored]
    if ref.numel():
        assert mag.max().item() <= 2048 < 2 ** 24 and ref.abs().max().item() <= 2048 and torch.equal(ref, ref.round())


# ---- a ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,u", M.KU)
def test_transposed_geometries_integer_operands_bit_exact(k, u):
    g = torch.Generator().manual_seed(1000 * k + u)
    bad = []
    for (cin, cout), ts in zip(UP_CH[(k, u)], UP_TS):
        for n, T in enumerate(ts):
            B = 1 + n % 2
            x, w, bias, Rr, old = int_operands(B, T, cin, cout, k, u, g)
            for arith in ARITHS:
                ref, mag, stored = model(arith, x, w, 1, u, 0.5, bias, Rr, old, 0.5, 2.0)
                assert stored.all() and ref.shape == (B, T * u, cout)
                assert_premise(ref, mag)
                out = run_layer(arith, _act(arith, x), w, 1, u, 0.5, bias, Rr, old, 0.5, 2.0)
                if not torch.equal(out, ref):
                    bad.append((arith, cin, cout, B, T, (out - ref).abs().max().item(), (out != ref).sum().item()))
    assert not bad, bad


# ---- b ------------------------------------------------------------------------------------------------------------------------------
RAGGED = [([0, 1, 127, 128, 129, 200, 9999], 1), ([0, 1, 43, 42, 9999], 3)]      # x len_mul: 0, 1, next to the tile edge, T, beyond T
SENTINEL = 7.0


def _ragged_case(k, dil, u, cin, cout, T, lens, len_mul, g):
    B = len(lens)
    x, w, bias, Rr, _ = int_operands(B, T, cin, cout, k, u, g)
    rows = [M.rows_of(lens, b, len_mul, T) for b in range(B)]
    for b, n in enumerate(rows):                     # nothing beyond an utterance's end may be read: neither x nor R
        x[b, n:] = NAN
        Rr[b, (n * u if u else n):] = NAN
    bad = []
    for arith in ARITHS:
        ref, mag, stored = model(arith, x, w, dil, u, 0.5, bias, Rr, None, 0.5, 0.0, lens=lens, len_mul=len_mul)
        assert_premise(ref, mag, stored)
        assert stored.sum(1).tolist() == [(n * u if u else n) for n in rows]
        fill = torch.full(ref.shape, SENTINEL, device=DEV)
        out = run_layer(arith, _act(arith, x), w, dil, u, 0.5, bias, Rr, fill, 0.5, 0.0, lens=lens, len_mul=len_mul)
        if out.isnan().any():
            bad.append((arith, "NaN", lens, len_mul))
        for b, n in enumerate(rows):
            no = n * u if u else n
            if n:
                alone = run_layer(arith, _act(arith, x[b:b + 1, :n]), w, dil, u, 0.5, bias, Rr[b:b + 1, :no].contiguous(), None, 0.5, 0.0)
                if not torch.equal(out[b, :no], ref[b, :no]):
                    bad.append((arith, "model", len_mul, b, n, (out[b, :no] - ref[b, :no]).abs().max().item()))
                if not torch.equal(out[b, :no], alone[0]):
                    bad.append((arith, "alone", len_mul, b, n))
            if not (out[b, no:] == SENTINEL).all():
                bad.append((arith, "stored beyond the end", len_mul, b, n))
    return bad


@pytest.mark.parametrize("k,u", M.KU)
def test_transposed_geometries_ragged(k, u):
    g = torch.Generator().manual_seed(2000 * k + u)
    cin, cout = UP_CH[(k, u)][M.KU.index((k, u)) % 2]
    bad = []
    for lens, len_mul in RAGGED:
        assert len(lens) >= 4
        bad += _ragged_case(k, 1, u, cin, cout, 200, lens, len_mul, g)
    assert not bad, bad


# ---- c ------------------------------------------------------------------------------------------------------------------------------
def input_forms(x):
    """x contiguous [B, T, C] -> the same values behind other strides and base pointers (NaN in every gap)"""
    B, T, C = x.shape
    chan_first = torch.empty(B, C, T, dtype=x.dtype, device=x.device).copy_(x.transpose(1, 2)).transpose(1, 2)      # sxc = T, sxt = 1
    big = torch.full((2 * B, T, C), NAN, dtype=x.dtype, device=x.device)
    big[::2] = x
    flat = torch.full((x.numel() + 1,), NAN, dtype=x.dtype, device=x.device)
    flat[1:] = x.reshape(-1)
    off1 = flat[1:].view(B, T, C)                                                # the base pointer one element past an aligned address
    assert off1.data_ptr() % 16 == x.element_size() and chan_first.stride(2) == T
    return {"channel-first": chan_first, "batch-strided": big[::2], "offset by one element": off1}


@pytest.mark.parametrize("k,dil", M.KD)
def test_conv1d_edges_and_input_forms_integer_operands(k, dil):
    g = torch.Generator().manual_seed(3000 * k + dil)
    bad = []
    for i, (cin, cout) in enumerate(CONV_CH):
        for n, T in enumerate(_conv_ts(i, k)):
            B = 1 + (i + n) % 2
            x, w, bias, Rr, old = int_operands(B, T, cin, cout, k, 0, g)
            for arith in ARITHS:
                ref, mag, stored = model(arith, x, w, dil, 0, 0.5, bias, Rr, old, 0.5, 2.0)
                assert_premise(ref, mag)
                xa = _act(arith, x)
                out = run_layer(arith, xa, w, dil, 0, 0.5, bias, Rr, old, 0.5, 2.0)
                if not torch.equal(out, ref):
                    bad.append((arith, "contiguous", cin, cout, B, T, (out - ref).abs().max().item()))
                forms = input_forms(xa)
                if arith == "fp16":
                    forms["float32 input"] = x                                    # rounded when staged: these integers are exact
                    forms["float32 channel-first"] = input_forms(x)["channel-first"]
                for name, xv in forms.items():
                    if not torch.equal(run_layer(arith, xv, w, dil, 0, 0.5, bias, Rr, old, 0.5, 2.0), out):
                        bad.append((arith, name, cin, cout, B, T))
    assert not bad, bad


@pytest.mark.parametrize("k,dil", [(3, 32), (65, 1), (7, 3)])
def test_conv1d_edges_ragged(k, dil):
    """the full halo with ragged ends (not in the issue's list for Conv1d; the walk and the bounds are the transposed conv's)"""
    g = torch.Generator().manual_seed(3500 * k + dil)
    bad = []
    for lens, len_mul in RAGGED:
        bad += _ragged_case(k, dil, 0, 20, 36, 200, lens, len_mul, g)
    assert not bad, bad


# ---- d ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,dil,u,cin,cout,T", [(7, 3, 0, 20, 36, 129), (12, 1, 4, 40, 24, 37)], ids=["conv1d", "transposed"])
def test_epilogue_all_sixteen_combinations(k, dil, u, cin, cout, T):
    g = torch.Generator().manual_seed(4000 + k)
    x, w, bias, Rr, old = int_operands(2, T, cin, cout, k, u, g)
    bad = []
    for mask in range(16):
        b_, r_ = (bias if mask & 1 else None), (Rr if mask & 2 else None)
        alpha, beta = (0.5 if mask & 4 else 1.0), (2.0 if mask & 8 else 0.0)
        prefill = old if beta else torch.full_like(old, NAN)                      # beta == 0: `out` must never be read
        for arith in ARITHS:                         # w, bias and R are even, so alpha = 0.5 keeps every term an integer
            ref, mag, _ = model(arith, x, w, dil, u, 0.5, b_, r_, old, alpha, beta)
            assert_premise(ref, mag)
            out = run_layer(arith, _act(arith, x), w, dil, u, 0.5, b_, r_, prefill, alpha, beta)
            if not torch.equal(out, ref):
                bad.append((arith, mask, (out - ref).abs().max().item(), out.isnan().sum().item()))
    assert not bad, bad


# ---- e ------------------------------------------------------------------------------------------------------------------------------
RANDOM = [(12, 1, 4, 20, 12), (12, 1, 4, 40, 24), (16, 1, 4, 20, 12), (16, 1, 4, 40, 24), (130, 1, 2, 20, 12), (130, 1, 2, 40, 24),
          (9, 1, 3, 16, 8), (3, 1, 1, 64, 48), (24, 1, 4, 40, 24),
          (3, 32, 0, 20, 36), (3, 32, 0, 33, 31), (65, 1, 0, 20, 36), (65, 1, 0, 33, 31), (7, 3, 0, 3, 5), (1, 1, 0, 36, 130), (17, 4, 0, 80, 100)]


@pytest.mark.parametrize("k,dil,u,cin,cout", RANDOM)
def test_random_operands_vs_fp64(k, dil, u, cin, cout):
    g = torch.Generator().manual_seed(5000 + 7 * k + cin)
    Kdim = (k // u if u else k) * cin
    for B, T in ((2, 129), (1, 37)):
        Tout = T * u if u else T
        x = torch.randn(B, T, cin, generator=g).to(DEV)
        w = (torch.randn((cin, cout, k) if u else (cout, cin, k), generator=g) / Kdim ** 0.5).to(DEV)
        bias = torch.randn(cout, generator=g).to(DEV)
        Rr = torch.randn(B, Tout, cout, generator=g).to(DEV)
        e = {}
        for arith in ("fp32", "split"):
            ref, _, _ = model(arith, x, w, dil, u, 0.1, bias, Rr)
            e[arith] = (run_layer(arith, x, w, dil, u, 0.1, bias, Rr) - ref).abs().max().item()
        floor = ULP * ref.abs().max().item()
        bar32 = 16 * floor * max(1.0, Kdim ** 0.5)
        xh, Rh = x.half(), Rr.half()
        refh, magh, _ = model("fp16", xh, w, dil, u, 0.1, bias, Rh)
        errh = (run_layer("fp16", xh, w, dil, u, 0.1, bias, Rh.float()) - refh).abs()
        limh = H.bound(refh, magh, Kdim)
        print(f"k={k} dil={dil} u={u} {cin}->{cout} B={B} T={T}: fp32 err {e['fp32']:.3e} (bar {bar32:.3e}), split err {e['split']:.3e} "
              f"(bar {1.25 * e['fp32'] + floor:.3e}), fp16 max err {errh.max().item():.3e}, largest err / bound {(errh / limh).max().item():.3f}")
        assert e["fp32"] <= bar32, e
        assert e["split"] <= 1.25 * e["fp32"] + floor, e
        assert (errh <= limh).all(), (B, T, (errh / limh).max().item())


# ---- f ------------------------------------------------------------------------------------------------------------------------------
REFUSED = [(3, 33, 0, "halo"), (67, 1, 0, "halo"), (9, 9, 0, "halo"), (132, 1, 2, "halo"),       # (taps - 1) x dil = 66, 66, 72, 65
           (4, 1, 0, "odd k"), (2, 3, 0, "odd k"),
           (5, 1, 2, "k % u"), (16, 1, 3, "k % u"),
           (6, 1, 3, "even"), (8, 1, 1, "even")]                                                 # k % u == 0, (k - u) odd


@pytest.mark.parametrize("k,dil,u,what", REFUSED)
def test_refused_geometries_raise_before_any_launch(k, dil, u, what):
    assert M.geometry(9, k, dil, u) is None
    B, T, cin, cout = 2, 9, 20, 12
    N, taps = (u * cout, k // u) if u else (cout, k)
    shape = (-(-N // 128) * 128, taps * 32)                                       # the shape the wrapper expects of the pack
    x = torch.ones(B, T, cin, device=DEV)
    for arith in ARITHS:
        out = torch.full((B, T * u if u else T, cout), NAN, dtype=torch.float16 if arith == "fp16" else torch.float32, device=DEV)
        with pytest.raises(_lib.CttsError, match=what):
            if arith == "fp16":
                K.vocoder_conv_h(x.half(), torch.ones(shape, dtype=torch.float16, device=DEV), cin, cout, k, dil, transposed_u=u, out=out)
            else:
                planes = torch.ones(shape[0], shape[1] // 32, 3, 32, dtype=torch.bfloat16, device=DEV) if arith == "split" else None
                K.vocoder_conv(x, torch.ones(shape, device=DEV), planes, cin, cout, k, dil, transposed_u=u, out=out,
                               bf16_split=1 if arith == "split" else 0)
        torch.cuda.synchronize()
        assert out.isnan().all(), arith                                           # untouched: nothing was launched


def test_generator_refuses_the_same_configs():
    V1 = H.V1
    for bad in (dict(upsample_rates=[8, 8, 2, 3], upsample_kernel_sizes=[16, 16, 4, 6]),       # k % u == 0, (k - u) odd
                dict(upsample_rates=[8, 8, 2, 1], upsample_kernel_sizes=[16, 16, 4, 8]),
                dict(upsample_kernel_sizes=[16, 16, 4, 132]),                                   # 66 taps
                dict(resblock_kernel_sizes=[3, 7, 4]),                                          # an even ResBlock kernel
                dict(resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 33]], resblock_kernel_sizes=[3, 7, 3]),     # halo 66
                dict(resblock_kernel_sizes=[3, 7, 67]),                                         # halo 66 at dilation 1
                dict(resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3]])):                  # the schedule needs three dilations
        with pytest.raises(NotImplementedError):
            Generator(AttrDict(dict(V1, **bad)))
    for ok in (dict(upsample_kernel_sizes=[16, 16, 4, 130]), dict(resblock_kernel_sizes=[3, 7, 65], resblock_dilation_sizes=[[1, 3, 5]] * 2 + [[1, 1, 1]]),
               dict(resblock_kernel_sizes=[3, 7, 3], resblock_dilation_sizes=[[1, 3, 5]] * 2 + [[1, 3, 32]])):
        Generator(AttrDict(dict(V1, upsample_initial_channel=32, **ok)))           # the edge of the contract is accepted


# ---- g ------------------------------------------------------------------------------------------------------------------------------
POST_C = [1, 8, 31, 32, 33, 80]
POST_T = [1, 3, 255, 256, 257, 600]
POST_ENDS = [([0, 1, 255, 256, 257, 600, 9999], 1), ([0, 85, 86, 9999], 3)]       # x len_mul: 0, 1, 255, 256, 257 / 258, T, beyond T


def run_post(half, x, w, bias, lens=None, len_mul=1):
    """ctts_vocoder_post / _post_ragged (fp32 x) or _post_h (fp16 x) into a NaN-prefilled `out` -> [B, T] float64"""
    B, T, _ = x.shape
    out = torch.full((B, 1, T), NAN, device=DEV)
    lt = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    res = (K.vocoder_post_h if half else K.vocoder_post)(x, w, bias, 0.01, out=out, lens=lt, len_mul=len_mul)
    assert res.data_ptr() == out.data_ptr() and res.dtype == torch.float32
    return res[:, 0].double()


def twin_error(pre):
    """the float32 twin of the last step: torch.tanh in float32 on the CPU of the float32-rounded pre-activation, against float64"""
    p = pre[~pre.isnan()].cpu()
    return (torch.tanh(p.float()).double() - torch.tanh(p)).abs().max().item() if p.numel() else 0.0


def post_bar(k, C, mag):
    return (k * C + 2) * 2.0 ** -24 * mag


@pytest.mark.parametrize("k", [1, 3, 7, 31])
def test_conv_post_dense_and_ragged_vs_fp64(k):
    g = torch.Generator().manual_seed(6000 + k)
    runs, twin = [], 0.0
    for C in POST_C:
        w = (1.5 * torch.randn(k, C, generator=g) / (k * C) ** 0.5).to(DEV)
        bias = (0.3 * torch.randn(1, generator=g)).to(DEV)
        for half in (False, True):
            for T in POST_T:
                x = torch.randn(2, T, C, generator=g).to(DEV)
                x = x.half() if half else x
                pre, mag, wav = M.conv_post(x, w, bias, 0.01)
                out = run_post(half, x, w, bias)
                twin = max(twin, twin_error(pre))
                runs.append(((C, half, T, "dense"), (out - wav).abs(), post_bar(k, C, mag), pre))
            T = 600
            for lens, len_mul in POST_ENDS:
                B = len(lens)
                x = torch.randn(B, T, C, generator=g).to(DEV)
                x = x.half() if half else x
                rows = [M.rows_of(lens, b, len_mul, T) for b in range(B)]
                for b, n in enumerate(rows):
                    x[b, n:] = NAN
                pre, mag, wav = M.conv_post(x, w, bias, 0.01, lens=lens, len_mul=len_mul)
                out = run_post(half, x, w, bias, lens, len_mul)
                assert not out.isnan().any(), (C, half, lens)
                for b, n in enumerate(rows):
                    assert (out[b, n:] == 0).all(), (C, half, b, n)                # exact zeros from the end on
                    if n:
                        alone = run_post(half, x[b:b + 1, :n].contiguous(), w, bias)
                        assert torch.equal(out[b, :n], alone[0]), (C, half, b, n)    # its own dense call, bit for bit
                twin = max(twin, twin_error(pre))
                valid = ~pre.isnan()
                runs.append(((C, half, lens, "ragged"), (out - wav).abs()[valid], post_bar(k, C, mag[valid]), pre[valid]))
    allow = 3.0 * twin                              # the allowance for the device's tanhf
    worst, worst_ratio, fails = 0.0, 0.0, []
    for name, err, bar, pre in runs:
        worst = max(worst, err.max().item())
        ratio = (err / (bar + allow)).max().item()
        worst_ratio = max(worst_ratio, ratio)
        if ratio > 1.0:
            fails.append((name, err.max().item(), ratio))
    print(f"conv_post k={k}: kernel max err {worst:.3e}, float32 twin max err {twin:.3e} (allowance {allow:.3e}), largest err / bar {worst_ratio:.3f}")
    assert not fails, fails


def test_conv_post_integer_operands():
    """pre-activations that are exact multiples of 1/8 in [-2, 2] (exact in fp32 in any order): a wrong tap or channel moves tanh by at
    least tanh(2) - tanh(1.875) = 9.9e-3, the bar is the tanhf allowance alone plus the (vacuous here) accumulation term"""
    g = torch.Generator().manual_seed(6100)
    for C, k, T in [(33, 7, 257), (31, 31, 300), (80, 3, 256), (1, 1, 3), (8, 7, 600)]:
        x = torch.tensor([-4.0, -2.0, 0.0, 1.0, 2.0, 3.0])[torch.randint(0, 6, (2, T, C), generator=g)].to(DEV)     # slope 0.5: |a| <= 3
        w = torch.zeros(k * C)
        w[torch.randperm(k * C, generator=g)[:4]] = (torch.randint(0, 2, (min(4, k * C),), generator=g) * 2 - 1).float() / 8
        w = w.reshape(k, C).to(DEV)
        bias = (torch.randint(-2, 3, (1,), generator=g).float() / 8).to(DEV)
        for half in (False, True):
            xa = x.half() if half else x
            pre, mag, wav = M.conv_post(xa, w, bias, 0.5)
            assert torch.equal(pre * 8, (pre * 8).round()) and pre.abs().max().item() <= 2.0 and pre.unique().numel() >= 3
            B = x.shape[0]
            out = torch.full((B, 1, T), NAN, device=DEV)
            (K.vocoder_post_h if half else K.vocoder_post)(xa, w, bias, 0.5, out=out)
            err = (out[:, 0].double() - wav).abs()
            lim = post_bar(k, C, mag) + 3.0 * twin_error(pre)
            print(f"conv_post integers C={C} k={k} T={T} half={half}: max err {err.max().item():.3e}, twin {twin_error(pre):.3e}")
            assert (err <= lim).all() and err.max().item() < 1e-6, (C, k, T, half, err.max().item())


# ---- h ------------------------------------------------------------------------------------------------------------------------------
CONFIGS = {"V2": dict(H.V1, upsample_initial_channel=128),
           "odd": dict(upsample_rates=[4, 2, 3], upsample_kernel_sizes=[12, 2, 9], upsample_initial_channel=48, resblock_kernel_sizes=[3, 5],
                       resblock_dilation_sizes=[[1, 2, 16], [1, 3, 5]], resblock="1")}
LENS = [11, 4]


def _generator(cfg, seed=11):
    """weights drawn as test_vocoder_gpu.py's _v1_generator draws them"""
    torch.manual_seed(seed)
    g = Generator(AttrDict(cfg))
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in g.named_modules():
            if hasattr(m, "weight_g"):
                m.weight_v.copy_(torch.randn(m.weight_v.shape, generator=gen))
                gain = (m.stride[0] * m.out_channels / m.in_channels) ** 0.5 if name.startswith("ups.") else (0.5 if name == "conv_post" else 1.0)
                m.weight_g.copy_(gain * (0.75 + 0.5 * torch.rand(m.weight_g.shape, generator=gen)))
                m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=gen))
    return g.eval()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(generator on the device, state dict, mel [2, 80, 11], float64 wav, the float32 CPU restatement's error) - computed once a config"""
    cfg = CONFIGS[name]
    g = _generator(cfg)
    sd = {k: v.detach().clone() for k, v in g.state_dict().items()}
    mel = torch.randn(2, 80, 11, generator=torch.Generator().manual_seed(2))
    ref = R.generator_forward(R.fold_state_dict(sd, dtype=torch.float64, device=DEV), cfg, mel.double().to(DEV)).cpu()
    with torch.no_grad():
        cpu32 = R.generator_forward(R.fold_state_dict(sd, dtype=torch.float32), cfg, mel)
    e_cpu = (cpu32.double() - ref).abs().max().item()
    assert 0.3 < ref.abs().max().item() < 0.9                                    # a waveform that is neither silent nor saturated
    return g.to(DEV), sd, mel, ref, e_cpu


def _hop(cfg):
    hop = 1
    for u in cfg["upsample_rates"]:
        hop *= u
    return hop


def _assert_ragged_is_each_utterance_alone(call, mel, hop):
    """test_vocoder_ragged_gpu.py's _assert_equals_alone at this generator's own hop, NaN in the padded frames"""
    B, _, T = mel.shape
    dirty = mel.clone()
    for b, n in enumerate(LENS):
        dirty[b, :, n:] = NAN
    wav = call(dirty, LENS)
    assert tuple(wav.shape) == (B, 1, hop * T) and torch.isfinite(wav).all()
    for b, n in enumerate(LENS):
        alone = call(mel[b:b + 1, :, :n], None)
        assert tuple(alone.shape) == (1, 1, hop * n) and torch.isfinite(alone).all()
        assert torch.equal(wav[b, 0, :hop * n], alone[0, 0]), (b, n, (wav[b, 0, :hop * n] - alone[0, 0]).abs().max().item())
        assert (wav[b, 0, hop * n:] == 0).all(), (b, n)
    return wav


@pytest.mark.parametrize("arith", ["split", "fp32"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_generator_other_geometries_vs_fp64_restatement(name, arith):
    g, sd, mel, ref, e_cpu = _reference(name)
    prev = K.gemm_bf16_split_enable(1 if arith == "split" else 0)
    try:
        out = g(mel.to(DEV), precision="fp32")
        assert out.shape == ref.shape and out.dtype == torch.float32
        e = (out.cpu().double() - ref).abs().max().item()
        print(f"{name} {arith} B=2 T=11: native err {e:.3e}, CPU fp32 restatement err {e_cpu:.3e}, wav peak {ref.abs().max().item():.3f}")
        wav = _assert_ragged_is_each_utterance_alone(lambda m, ln: g(m, lens=ln, precision="fp32"), mel.to(DEV), _hop(CONFIGS[name]))
        assert torch.equal(wav[0], out[0])                                        # the full-length utterance is the dense one
    finally:
        K.gemm_bf16_split_enable(prev)
    assert e <= 2 * e_cpu, (e, e_cpu)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_generator_other_geometries_fp16(name):
    g, sd, mel, ref, _ = _reference(name)
    H._against_fp64(f"{name} B=2 T=11", g, CONFIGS[name], sd, mel)
    wav = _assert_ragged_is_each_utterance_alone(lambda m, ln: g(m, lens=ln, precision="fp16"), mel.to(DEV), _hop(CONFIGS[name]))
    assert torch.equal(wav[0], g(mel.to(DEV), precision="fp16")[0])
