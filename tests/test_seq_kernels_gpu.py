"""GPU: the sequence kernels of the Conformer block and of the prosody encoders - GLU, depthwise Conv1d (forward, data gradient,
weight gradient) and relattn_split (csrc/conformer.hip), the four GRU kernels and the Conv2d patch kernels im2col_3x3s2 / col2im_3x3s2
(csrc/prosody.hip) - against the float64 restatement tests/seq_restate64.py, at the sizes where their grids, chunking, prefetch
buffers and code paths change.

Error measure (never the tensor's global maximum):
  * GRU out, gates (each of r, z, n, W_hn h + b_hn on its own), dgi, dgh: per (b, t, direction) row, max |got - ref64| over the row
    divided by the row's reference RMS; a reference row of zeros must be met exactly.  With saturated gates the gradients are
    measured per (b, direction) slab instead (rows of exactly saturated steps are about 0 in float32 and in the kernel alike).
  * sums - depthwise y / dx / dw, col2im, dW_hh, db_hh and the GEMM-made dx, dW_ih, db_ih of ops.gru: element by element against
    the L2 norm of the float64 summands (an accumulating call: plus |old|).
  * GLU: element by element against |x| (forward), |dout| (x half of the gradient) and |dout * x| (gate half).
  * copies are bit-exact: im2col, hprev (= the kernel's own out shifted one processed step, zeros at the first processed step), the kv
    half of relattn_split and its two single float32 adds (against the same adds in torch float32).

Bar of every measured quantity: max(FACTOR x the error of the same restatement run in float32 on the CPU (same input, same measure),
4 * 2^-23).  FACTOR = 8 and the floor are the constants of tests/test_norm_kernels_gpu.py (a different summation order, the hardware
__expf / __frcp_rn, the final rounding); the 8 is the project's convention, INHERITED and not measured for these kernels.  Every
comparison prints `kernel err / stock float32 err / bar` (run with -s).

No GRU quantity needed a wider factor: the largest kernel / float32 ratio of any GRU row measure is 4.5 (dgi, H = 16, T = 25), the error
does not grow with T (out per block of 100 steps at T = 600: 4.9e-7 ... 6.0e-7 against 3.4e-7 ... 5.6e-7 for float32) and the two H = 32
kernels differ by at most 2.4e-6 (dgh, T = 24) where the sum of their bars is 1.7e-5.  GRU_FACTOR stays empty.

Measured on the MI355X, worst case per quantity (kernel error / stock float32 error / bar; 851 comparisons, none above 0.56 of its bar):
  GRU kernels, T <= 25   out 7.4e-7 / 3.5e-7 / 2.8e-6   r 1.9e-7 / 1.6e-7 / 1.3e-6   z 2.2e-7 / 1.5e-7 / 1.2e-6   n 5.4e-7 / 1.7e-7 / 1.4e-6
  and the masks          W_hn h + b_hn 2.2e-6 / 5.6e-7 / 4.5e-6 (H 128: 4.0 x float32)   dgi 4.0e-6 / 9.0e-7 / 7.2e-6 (H 16, T 9)
                         dgh 2.9e-6 / 1.1e-6 / 9.1e-6 (H 32 one-wave, mask 0b101)   n at T = 1, H 64: 4.2 x float32 (tanh as 1 - 2 / (1 + e^2v))
  GRU, T = 600           out 6.0e-7 / 5.6e-7 / 4.5e-6   dgi 2.3e-6 / 1.6e-6 / 1.3e-5
  GRU, saturated gates   r 2.7e-7 / 1.5e-7 / 1.2e-6 (H 128, +-15)   per slab: dgi 5.4e-6 / 3.4e-6 / 2.8e-5   dgh 5.4e-6 / 4.5e-6 / 3.6e-5
  ops.gru / gru_group    dx 1.1e-6 / 1.3e-6 / 1.1e-5   dW_ih 3.9e-6 / 1.1e-5 / 8.6e-5   db_ih, db_hh 2.6e-6 / 8.0e-6 / 6.4e-5 (all three at T = 1)
                         dW_hh 1.4e-6 / 1.7e-6 / 1.4e-5 (exactly 0 at T = 1)
  depthwise conv         y 8.4e-7 / 8.4e-7 / 6.8e-6   y halo 7.5e-7 / 7.5e-7 / 6.0e-6   dx 9.6e-7 / 7.6e-7 / 6.1e-6   dx halo 7.7e-7 / 6.2e-7 / 4.9e-6
                         dw 8.4e-7 / 6.3e-7 / 5.1e-6 (260 chunks, C 384, K 31)   dw accumulated 8.2e-7 / 7.0e-7 / 5.6e-6
                         (largest dw ratio 1.5 x float32 at 127 chunks, C 384, K 7)
  GLU                    out 1.4e-7 / 1.4e-7 / 1.2e-6   dx 1.5e-7 / 1.5e-7 / 1.2e-6   dgate 8.9e-8 / 8.9e-8 / 7.1e-7
  Conv2d patches         col2im 1.9e-7 / 1.9e-7 / 1.6e-6   last column of an even W 8.3e-8 / 8.3e-8 / 6.6e-7
                         ops.conv2d_3x3s2: y 1.4e-6 / 6.6e-7 / 5.3e-6   dx 4.3e-7 / 4.4e-7 / 3.5e-6
  bit-exact              im2col, hprev, relattn_split (qu, qv, kv, dqkv) at every shape
"""
import functools
import math

import pytest
import torch

import ctts_amd  # noqa: F401
from ctts_amd import kernels as K
from ctts_amd import ops
from ctts_amd._lib import CttsError
from tests import seq_restate64 as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 4 * 2.0 ** -23
FACTOR = 8.0
TINY = 1e-300
D, F32 = torch.float64, torch.float32


def dev(t):
    return t.to(DEV)


def c64(t):
    return t.detach().double().cpu()


def err_rows(got, ref64, dim=-1, scale_of=None):
    """worst over the rows of max |got - ref64| / RMS(scale_of or ref64), both taken along `dim` (a tuple: a slab)"""
    got, ref64 = c64(got), c64(ref64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    if ref64.numel() == 0:
        return 0.0
    rms = (ref64 if scale_of is None else c64(scale_of)).pow(2).mean(dim).sqrt()
    return ((got - ref64).abs().amax(dim) / rms.clamp_min(TINY)).max().item()


def err_scaled(got, ref64, scale):
    """worst |got - ref64| / scale, element for element (scale 0: the element must be met exactly)"""
    got, ref64 = c64(got), c64(ref64)
    assert got.shape == ref64.shape == scale.shape, (got.shape, ref64.shape, scale.shape)
    return ((got - ref64).abs() / scale.double().clamp_min(TINY)).max().item() if got.numel() else 0.0


def bar_of(e32, factor=FACTOR):
    return max(factor * e32, FLOOR)


def judge(name, e, e32, factor=FACTOR):
    bar = bar_of(e32, factor)
    print(f"{name}: kernel err {e:.2e}  stock float32 {e32:.2e}  bar {bar:.2e}")
    assert math.isfinite(e) and e <= bar, f"{name}: kernel err {e:.3e} > bar {bar:.3e} (stock float32 {e32:.3e})"
    return bar


def check_rows(name, got, r64, r32, dim=-1, factor=FACTOR):
    assert torch.isfinite(got).all(), name
    return judge(name, err_rows(got, r64, dim), err_rows(r32, r64, dim), factor)


def check_scaled(name, got, r64, r32, scale, factor=FACTOR):
    assert torch.isfinite(got).all(), name
    return judge(name, err_scaled(got, r64, scale), err_scaled(r32, r64, scale), factor)


# ================================================================================================ GRU
GRU_B = 3
KERNELS = {"h16": (16, False), "h32_wave": (32, False), "h32_multi": (32, True), "h64": (64, False), "h128": (128, False)}
CHUNK_T = (1, 2, 7, 8, 9, 15, 16, 17, 24, 25)        # partial chunk / one chunk / second buffer / two chunks / back to the first buffer
GRU_FACTOR = {}                                       # quantity -> widened factor (none: see the module docstring)


@functools.lru_cache(maxsize=None)
def gru_ref(T, H, ndir, mask, dtype, seed=0, gi_scale=1.0, spike=0.0):
    i = S.gru_inputs(GRU_B, T, H, ndir, seed, gi_scale, spike)
    return S.gru(i["gi"], i["whh"], i["bhh"], mask, i["dout"], dtype=dtype)


def select_kernel(monkeypatch, multi):
    if multi:
        monkeypatch.setenv("CTTS_GRU_MULTIWAVE", "1")
    else:
        monkeypatch.delenv("CTTS_GRU_MULTIWAVE", raising=False)


def gru_kernel(i, H, ndir, mask):
    B, T = i["gi"].shape[:2]
    whh = dev(i["whh"])
    out, gates = K.gru_fwd(dev(i["gi"]).view(B, T, ndir * 3 * H), whh, dev(i["bhh"]), H, ndir, True, mask)
    dgi, dgh, hprev = K.gru_bwd(dev(i["dout"]).view(B, T, ndir * H), out, gates, whh, H, ndir, mask)
    return dict(out=out.view(B, T, ndir, H), gates=gates.view(B, T, ndir, 4 * H), dgi=dgi.view(B, T, ndir, 3 * H),
                dgh=dgh.view(B, T, ndir, 3 * H), hprev=hprev.view(B, T, ndir, H))


def shifted_out(out, mask):
    """[B,T,ndir,H]: out one processed step earlier, zeros at the first processed step"""
    want = torch.zeros_like(out)
    for d in range(out.shape[2]):
        if (mask >> d) & 1:
            want[:, :-1, d] = out[:, 1:, d]
        else:
            want[:, 1:, d] = out[:, :-1, d]
    return want


def gru_compare(tag, k, r64, r32, mask, quantities=("out", "gates", "dgi", "dgh")):
    bars = {}
    H = k["out"].shape[-1]
    for q in quantities:
        f = GRU_FACTOR.get(q, FACTOR)
        if q == "gates":
            for j, g in enumerate(("r", "z", "n", "ghn")):
                sl = slice(j * H, (j + 1) * H)
                bars[g] = check_rows(f"gru {g} [{tag}]", k[q][..., sl], r64[q][..., sl], r32[q][..., sl], factor=GRU_FACTOR.get(g, FACTOR))
        else:
            bars[q] = check_rows(f"gru {q} [{tag}]", k[q], r64[q], r32[q], factor=f)
    assert torch.equal(k["hprev"], shifted_out(k["out"], mask)), f"{tag}: hprev is not out shifted one processed step"
    return bars


GRU_CASES = [(kn, ndir, T) for kn in KERNELS for ndir in (1, 2) for T in (CHUNK_T if KERNELS[kn][0] <= 32 else (1, 9, 25))]


@pytest.mark.parametrize("kernel,ndir,T", GRU_CASES)
def test_gru_kernels_against_float64(kernel, ndir, T, monkeypatch):
    """every kernel at one step, a chunk and a step, three chunks and a step; the H = 16 and both H = 32 kernels at every length
    around the 8-step prefetch chunk and its double-buffer swap; one direction, and forward | reversed"""
    H, multi = KERNELS[kernel]
    select_kernel(monkeypatch, multi)
    mask = 2 if ndir == 2 else 0
    k = gru_kernel(S.gru_inputs(GRU_B, T, H, ndir), H, ndir, mask)
    gru_compare(f"{kernel} ndir {ndir} T {T}", k, gru_ref(T, H, ndir, mask, D), gru_ref(T, H, ndir, mask, F32), mask)


@pytest.mark.parametrize("T", CHUNK_T)
def test_gru_both_h32_kernels_agree(T, monkeypatch):
    """one-wave and multi-wave H = 32: each within its bar, and their difference within the sum of the two bars (same measure)"""
    i = S.gru_inputs(GRU_B, T, 32, 2)
    r64, r32 = gru_ref(T, 32, 2, 2, D), gru_ref(T, 32, 2, 2, F32)
    select_kernel(monkeypatch, False)
    kw = gru_kernel(i, 32, 2, 2)
    select_kernel(monkeypatch, True)
    km = gru_kernel(i, 32, 2, 2)
    for q in ("out", "dgi", "dgh"):
        bar = bar_of(err_rows(r32[q], r64[q]), GRU_FACTOR.get(q, FACTOR))
        e = err_rows(kw[q], km[q], scale_of=r64[q])
        print(f"gru h32 wave-vs-multi {q} [T {T}]: difference {e:.2e}  sum of bars {2 * bar:.2e}")
        assert e <= 2 * bar, f"{q} T {T}: the two H = 32 kernels differ by {e:.3e} > {2 * bar:.3e}"


@pytest.mark.parametrize("ndir,mask", [(2, 0), (1, 1), (3, 0b101)])
@pytest.mark.parametrize("kernel", ["h32_wave", "h16"])
def test_gru_direction_masks(kernel, ndir, mask, monkeypatch):
    """two forward sequences (the gru_group layout), one reversed sequence, three sequences reversed | forward | reversed"""
    H, multi = KERNELS[kernel]
    select_kernel(monkeypatch, multi)
    T = 9
    k = gru_kernel(S.gru_inputs(GRU_B, T, H, ndir, seed=mask + 1), H, ndir, mask)
    gru_compare(f"{kernel} ndir {ndir} mask {mask:#b} T {T}", k, gru_ref(T, H, ndir, mask, D, mask + 1), gru_ref(T, H, ndir, mask, F32, mask + 1),
                mask)


def test_gru_long_recurrence_stays_within_the_bar_at_every_step(monkeypatch):
    """T = 600 (the reference-encoder recurrences run over mel frames): the worst row over all steps is judged, and printed per
    block of 100 steps"""
    select_kernel(monkeypatch, False)
    T = 600
    k = gru_kernel(S.gru_inputs(GRU_B, T, 32, 1, seed=5), 32, 1, 0)
    r64, r32 = gru_ref(T, 32, 1, 0, D, 5), gru_ref(T, 32, 1, 0, F32, 5)
    for q in ("out", "dgi"):
        for t0 in range(0, T, 100):
            print(f"  steps {t0}..{t0 + 99} {q}: kernel {err_rows(k[q][:, t0:t0 + 100], r64[q][:, t0:t0 + 100]):.2e}  "
                  f"stock float32 {err_rows(r32[q][:, t0:t0 + 100], r64[q][:, t0:t0 + 100]):.2e}")
    gru_compare("h32_wave ndir 1 T 600", k, r64, r32, 0)


@pytest.mark.parametrize("gi_scale,spike", [(5.0, 0.0), (1.0, 200.0)], ids=["pre15", "spike200"])
@pytest.mark.parametrize("kernel", ["h32_wave", "h32_multi", "h128"])
def test_gru_saturated_gates(kernel, gi_scale, spike, monkeypatch):
    """pre-activations of about +-15, and entries of +-200 (__expf overflows to inf, 1 / inf = 0): everything finite, the forward
    within the bar row by row, the gradients within the bar per (b, direction) slab"""
    H, multi = KERNELS[kernel]
    select_kernel(monkeypatch, multi)
    T, ndir, mask = 17, 2, 2
    k = gru_kernel(S.gru_inputs(GRU_B, T, H, ndir, 7, gi_scale, spike), H, ndir, mask)
    r64, r32 = gru_ref(T, H, ndir, mask, D, 7, gi_scale, spike), gru_ref(T, H, ndir, mask, F32, 7, gi_scale, spike)
    assert r64["gates"][..., :2 * H].max() > 1 - 1e-6 and r64["gates"][..., :2 * H].min() < 1e-6, "the test needs saturated gates"
    for q in k:
        assert torch.isfinite(k[q]).all(), q
    tag = f"{kernel} saturated {'spike 200' if spike else 'pre 15'}"
    gru_compare(tag, k, r64, r32, mask, quantities=("out", "gates"))
    for q in ("dgi", "dgh"):
        judge(f"gru {q} per slab [{tag}]", err_rows(k[q], r64[q], (1, 3)), err_rows(r32[q], r64[q], (1, 3)), GRU_FACTOR.get(q, FACTOR))


def l2(t, dims):
    return t.double().pow(2).sum(dims).sqrt()


def gru_op_ref(x, wih, bih, whh, bhh, dout, mask, dtype):
    """x [B,T,In], wih [ndir,3H,In], bih [ndir,3H] -> the oracle's GRU on gi = W_ih x + b_ih plus dx, dW_ih, db_ih with summand norms"""
    x, wih, bih = x.to(dtype), wih.to(dtype), bih.to(dtype)
    gi = torch.einsum("bti,dgi->btdg", x, wih) + bih
    r = S.gru(gi, whh, bhh, mask, dout, dtype=dtype)
    g = r["dgi"]
    r.update(dx=torch.einsum("btdg,dgi->bti", g, wih), dx_norm=torch.einsum("btdg,dgi->bti", g * g, wih * wih).sqrt(),
             dwih=torch.einsum("btdg,bti->dgi", g, x), dwih_norm=torch.einsum("btdg,bti->dgi", g * g, x * x).sqrt(),
             dbih=g.sum((0, 1)), dbih_norm=(g * g).sum((0, 1)).sqrt())
    return r


@pytest.mark.parametrize("T", [17, 1])
def test_ops_gru_bidirectional_gradients_against_float64(T, monkeypatch):
    """ops.gru through autograd: dx, dW_ih, db_ih (GEMMs and column sums over dgi), dW_hh (split-K GEMM over B * T rows, nearly empty at
    T = 1 where h_prev = 0 and dW_hh must be exactly 0) and db_hh"""
    select_kernel(monkeypatch, False)
    B, H, In = GRU_B, 32, 48
    i = S.gru_inputs(B, T, H, 2, seed=11)
    g = torch.Generator().manual_seed(T)
    x = torch.randn(B, T, In, generator=g)
    wih, bih = (torch.rand(2, 3 * H, In, generator=g) * 2 - 1) * H ** -0.5, (torch.rand(2, 3 * H, generator=g) * 2 - 1) * H ** -0.5
    r64, r32 = [gru_op_ref(x, wih, bih, i["whh"], i["bhh"], i["dout"], 2, t) for t in (D, F32)]
    xd = dev(x).requires_grad_()
    prm = [dev(t[d]).clone().requires_grad_() for d in range(2) for t in (wih, i["whh"], bih, i["bhh"])]
    out = ops.gru(xd, *prm)
    out.backward(dev(i["dout"]).view(B, T, 2 * H))
    tag = f"ops.gru T {T}"
    check_rows(f"gru out [{tag}]", out.view(B, T, 2, H), r64["out"], r32["out"], factor=GRU_FACTOR.get("out", FACTOR))
    check_scaled(f"gru dx [{tag}]", xd.grad, r64["dx"], r32["dx"], r64["dx_norm"])
    for q, j in (("dwih", 0), ("dwhh", 1), ("dbih", 2), ("dbhh", 3)):
        got = torch.stack([prm[j].grad, prm[4 + j].grad])
        check_scaled(f"gru {q} [{tag}]", got, r64[q], r32[q], r64[q + "_norm"])
    if T == 1:
        assert (prm[1].grad == 0).all() and (prm[5].grad == 0).all()


def test_ops_gru_group_against_float64(monkeypatch):
    """ops.gru_group: two forward GRUs in one launch (rev_mask 0, ndir 2)"""
    select_kernel(monkeypatch, False)
    B, T, H = GRU_B, 17, 32
    i = S.gru_inputs(B, T, H, 2, seed=12)
    r64, r32 = [S.gru(i["gi"], i["whh"], i["bhh"], 0, i["dout"], dtype=t) for t in (D, F32)]
    gis = [dev(i["gi"][:, :, d]).clone().requires_grad_() for d in range(2)]
    whhs = [dev(i["whh"][d]).clone().requires_grad_() for d in range(2)]
    bhhs = [dev(i["bhh"][d]).clone().requires_grad_() for d in range(2)]
    outs = ops.gru_group(gis, whhs, bhhs)
    sum((o * dev(i["dout"][:, :, d])).sum() for d, o in enumerate(outs)).backward()
    tag = "ops.gru_group T 17"
    check_rows(f"gru out [{tag}]", torch.stack(list(outs), 2), r64["out"], r32["out"], factor=GRU_FACTOR.get("out", FACTOR))
    check_rows(f"gru dgi [{tag}]", torch.stack([t.grad for t in gis], 2), r64["dgi"], r32["dgi"], factor=GRU_FACTOR.get("dgi", FACTOR))
    check_scaled(f"gru dwhh [{tag}]", torch.stack([t.grad for t in whhs]), r64["dwhh"], r32["dwhh"], r64["dwhh_norm"])
    check_scaled(f"gru dbhh [{tag}]", torch.stack([t.grad for t in bhhs]), r64["dbhh"], r32["dbhh"], r64["dbhh_norm"])


def test_gru_bwd_unsupported_hidden_size_fails_loudly():
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(CttsError):
        K.gru_bwd(z(1, 2, 24), z(1, 2, 24), z(1, 2, 96), z(1, 72, 24), 24, 1)


# ================================================================================================ depthwise conv
def dw_groups(C):
    return max(1, 256 // (C // 4))


def dw_fwd_cases():
    cases = [(256, K_, 2, T) for K_ in (31, 7, 1) for T in (1, 7, 8, 9, 15, 16, 31, 32, 33, 64, 65)]
    for C, K_ in ((80, 31), (384, 31), (1024, 15)):
        g8 = dw_groups(C) * 8
        cases += [(C, K_, 2, T) for T in (1, g8 - 1, g8, g8 + 1)]
    return cases + [(4, 3, 1, T) for T in (1, 2047, 2048, 2049)]


@functools.lru_cache(maxsize=None)
def dw_ref(B, T, C, K_, dtype, seed=0):
    i = S.dw_inputs(B, T, C, K_, seed)
    return S.dwconv(i["x"], i["w"], i["dy"], dtype=dtype)


@pytest.mark.parametrize("C,K_,B,T", dw_fwd_cases())
def test_dwconv_forward_and_data_gradient_against_float64(C, K_, B, T):
    """C / 4 lanes x `groups` time groups of 8 steps per block: T around 8 and around groups * 8, 240- and 192-thread blocks, one
    block over 2048 steps (C = 4), the tap guard and the row mask for K < 31, K = 1; the halo rows also on their own"""
    i = S.dw_inputs(B, T, C, K_)
    r64, r32 = dw_ref(B, T, C, K_, D), dw_ref(B, T, C, K_, F32)
    wT = dev(i["w"]).t().contiguous()
    pad = (K_ - 1) // 2
    halo = torch.arange(T)
    halo = (halo < pad) | (halo >= T - pad)
    for q, src, flip in (("y", "x", False), ("dx", "dy", True)):
        got = K.dwconv_fwd(dev(i[src]), wT, flip)
        tag = f"[C {C} K {K_} B {B} T {T}]"
        check_scaled(f"dwconv {q} {tag}", got, r64[q], r32[q], r64[q + "_norm"])
        if halo.any():
            check_scaled(f"dwconv {q} halo {tag}", got[:, dev(halo)], r64[q][:, halo], r32[q][:, halo], r64[q + "_norm"][:, halo])


# chunks = B * ceil(T / 32), cut into at most 128 slices of `per` chunks
DW_WGRAD_BT = {1: (1, 20), 7: (1, 221), 8: (2, 100), 9: (3, 70), 127: (1, 4059), 128: (2, 2048), 129: (3, 1370), 260: (4, 2080)}
DW_WGRAD_CASES = ([(n, 256, 31) for n in DW_WGRAD_BT] + [(n, 384, 7) for n in DW_WGRAD_BT] + [(129, 256, 7), (129, 384, 31), (260, 384, 31)])


@pytest.mark.parametrize("chunks,C,K_", DW_WGRAD_CASES)
def test_dwconv_weight_gradient_against_float64(chunks, C, K_):
    """per = 1 with 1 .. 128 slices (the reducer's unrolled-by-8 loop: tail only, one trip, trip + tail, 15 trips + 7, 16 trips), per = 2
    with slices that span two utterances at T % 32 != 0 (129 chunks), per = 3 with empty trailing slices (260); C = 384 runs the
    second, half-idle blockIdx.y; K = 7 must not see taps 7 .. 31 of the partials.  Then the accumulating call (old + gradient, and
    nothing written past C * K floats), and a repeat that must be bit-identical."""
    B, T = DW_WGRAD_BT[chunks]
    assert B * ((T + 31) // 32) == chunks
    i = S.dw_inputs(B, T, C, K_, seed=1)
    r64, r32 = dw_ref(B, T, C, K_, D, 1), dw_ref(B, T, C, K_, F32, 1)
    dy, x = dev(i["dy"]), dev(i["x"])
    tag = f"[chunks {chunks} B {B} T {T} C {C} K {K_}]"
    dw = K.dwconv_wgrad(dy, x, K_)
    assert dw.shape == (C, K_)
    check_scaled(f"dwconv dw {tag}", dw, r64["dw"], r32["dw"], r64["dw_norm"])
    assert torch.equal(K.dwconv_wgrad(dy, x, K_), dw), "two identical calls differ"
    sentinel = -12345.678
    buf = torch.full((C * K_ + 64,), sentinel, device=DEV)
    acc = buf[:C * K_].view(C, K_)
    acc.copy_(dev(i["old"]))
    assert K.dwconv_wgrad(dy, x, K_, acc_into=acc) is None
    assert (buf[C * K_:] == sentinel).all(), "the accumulating call wrote past C * K floats"
    old = i["old"].double()
    check_scaled(f"dwconv dw accumulated {tag}", acc, old + r64["dw"], i["old"] + r32["dw"], r64["dw_norm"] + old.abs())


def test_ops_depthwise_conv1d_against_float64():
    """ops.depthwise_conv1d through autograd, w in the nn.Conv1d [C,1,K] layout; then with gradient-accumulation fusion, where the
    weight gradient is added to an existing w.grad by the kernel"""
    B, T, C, K_ = 2, 97, 80, 31
    i = S.dw_inputs(B, T, C, K_, seed=2)
    r64, r32 = dw_ref(B, T, C, K_, D, 2), dw_ref(B, T, C, K_, F32, 2)
    x, w = dev(i["x"]).requires_grad_(), dev(i["w"]).view(C, 1, K_).clone().requires_grad_()
    y = ops.depthwise_conv1d(x, w)
    y.backward(dev(i["dy"]))
    tag = f"[ops C {C} K {K_} B {B} T {T}]"
    check_scaled(f"dwconv y {tag}", y, r64["y"], r32["y"], r64["y_norm"])
    check_scaled(f"dwconv dx {tag}", x.grad, r64["dx"], r32["dx"], r64["dx_norm"])
    check_scaled(f"dwconv dw {tag}", w.grad.view(C, K_), r64["dw"], r32["dw"], r64["dw_norm"])
    was = ops.grad_accumulation_fusion()
    ops.set_grad_accumulation_fusion(True)
    try:
        w2 = dev(i["w"]).view(C, 1, K_).clone().requires_grad_()
        w2.grad = dev(i["old"]).view(C, 1, K_).clone()
        ops.depthwise_conv1d(dev(i["x"]), w2).backward(dev(i["dy"]))
    finally:
        ops.set_grad_accumulation_fusion(was)
    old = i["old"].double()
    check_scaled(f"dwconv dw accumulated {tag}", w2.grad.view(C, K_), old + r64["dw"], i["old"] + r32["dw"], r64["dw_norm"] + old.abs())


@pytest.mark.parametrize("C,K_", [(256, 4), (256, 33), (6, 3), (1028, 3), (1024, 31)],
                         ids=["even_K", "K_33", "C_not_x4", "C_1028", "weights_over_64KiB"])
def test_dwconv_forward_rejects_what_it_cannot_run(C, K_):
    with pytest.raises(CttsError):
        K.dwconv_fwd(torch.zeros(1, 8, C, device=DEV), torch.zeros(K_, C, device=DEV))


@pytest.mark.parametrize("K_", [4, 33])
def test_dwconv_weight_gradient_rejects_even_and_oversized_K(K_):
    with pytest.raises(CttsError):
        K.dwconv_wgrad(torch.zeros(1, 8, 256, device=DEV), torch.zeros(1, 8, 256, device=DEV), K_)


# ================================================================================================ GLU, relattn_split
# 8193 rows x 1024 channels / 10923 rows x 3 * 256 channels: the smallest row counts with more than 8192 * 256 float4 elements, so that
# the grid-stride loop of the capped grid takes a second trip
@pytest.mark.parametrize("rows,C", [(1, 4), (135, 256), (7, 1024), (8193, 1024)])
def test_glu_against_float64(rows, C):
    """gates include +-30 and +-100: sigmoid is measured absolutely, against |x|; everything finite"""
    i = S.glu_inputs(rows, C)
    r64, r32 = [S.glu(i["a"], i["dout"], dtype=t) for t in (D, F32)]
    a = dev(i["a"])
    out, da = K.glu_fwd(a), K.glu_bwd(a, dev(i["dout"]))
    x, d = i["a"][:, :C].double(), i["dout"].double()
    tag = f"[{rows}, {C}]"
    check_scaled(f"glu out {tag}", out, r64["out"], r32["out"], x.abs())
    check_scaled(f"glu dx {tag}", da[:, :C], r64["da"][:, :C], r32["da"][:, :C], d.abs())
    check_scaled(f"glu dgate {tag}", da[:, C:], r64["da"][:, C:], r32["da"][:, C:], (d * x).abs())


def test_ops_glu_autograd_is_the_kernel_pair():
    i = S.glu_inputs(135, 256, seed=1)
    a = dev(i["a"]).requires_grad_()
    out = ops.glu(a)
    out.backward(dev(i["dout"]))
    assert torch.equal(out, K.glu_fwd(a.detach())) and torch.equal(a.grad, K.glu_bwd(a.detach(), dev(i["dout"])))


@pytest.mark.parametrize("rows,C", [(1, 4), (135, 256), (10923, 256)])
def test_relattn_split_is_bit_exact(rows, C):
    i = S.split_inputs(rows, C)
    qu, qv, kv = K.relattn_split_fwd(dev(i["qkv"]), dev(i["u"]), dev(i["v"]))
    wu, wv, wkv = S.relattn_split(i["qkv"], i["u"], i["v"], F32)
    assert torch.equal(kv.cpu(), wkv), "kv is a copy"
    assert torch.equal(qu.cpu(), wu) and torch.equal(qv.cpu(), wv), "qu / qv are single float32 adds"
    dqkv = K.relattn_split_bwd(dev(i["dqu"]), dev(i["dqv"]), dev(i["dkv"]))
    assert torch.equal(dqkv.cpu(), S.relattn_split_bwd(i["dqu"], i["dqv"], i["dkv"], F32)), "dqkv = (dqu + dqv) | dkv, one float32 add"
    print(f"relattn_split [{rows}, {C}]: bit-exact ({3 * rows * C // 4} float4 elements)")


# ================================================================================================ Conv2d patches
PATCH_SHAPES = [(1, 1, 1, 4), (2, 1, 2, 4), (2, 2, 3, 32), (1, 3, 4, 32), (2, 2, 5, 4), (1, 3, 80, 4)]


@pytest.mark.parametrize("B,T,W,C", PATCH_SHAPES)
def test_im2col_is_bit_exact_and_col2im_against_float64(B, T, W, C):
    """W = 1, 2, 4: one output column, and even widths whose last input column is read through kw = 2 only; T = 1, 2: every row sees
    the padding above and below"""
    i = S.patch_inputs(B, T, W, C)
    col = K.im2col_3x3s2(dev(i["x"]))
    assert torch.equal(col.cpu(), S.im2col_3x3s2(i["x"])), "im2col is a gather"
    dx = K.col2im_3x3s2(dev(i["dcol"]), B, T, W, C)
    (d64, n64), (d32, _) = [S.col2im_3x3s2(i["dcol"], B, T, W, C, dtype=t) for t in (D, F32)]
    tag = f"[{B}, {T}, {W}, {C}]"
    check_scaled(f"col2im dx {tag}", dx, d64, d32, n64)
    if W % 2 == 0:
        assert (n64[:, :, W - 1] > 0).all()
        check_scaled(f"col2im dx last column {tag}", dx[:, :, W - 1], d64[:, :, W - 1], d32[:, :, W - 1], n64[:, :, W - 1])


def test_ops_conv2d_3x3s2_against_float64():
    """ops.conv2d_3x3s2 forward / backward at an even width: y and dx with the sum measure (dx sums Cout x at most 6 products)"""
    B, T, W, Cin, Cout = 2, 2, 4, 32, 32
    Wo = (W - 1) // 2 + 1
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(B, T, W, Cin, generator=g), torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1, torch.randn(Cout, generator=g)
    dy = torch.randn(B, T, Wo, Cout, generator=g)

    def ref(dtype):
        xs, wf, d = x.to(dtype), w.to(dtype).permute(0, 2, 3, 1).reshape(Cout, 9 * Cin), dy.to(dtype).reshape(-1, Cout)
        col = S.im2col_3x3s2(xs)
        y = col @ wf.t() + b.to(dtype)
        y_norm = ((col * col) @ (wf * wf).t() + b.to(dtype) ** 2).sqrt()
        dx, _ = S.col2im_3x3s2(d @ wf, B, T, W, Cin, dtype=dtype)
        dx_norm = S.col2im_3x3s2((d * d) @ (wf * wf), B, T, W, Cin, dtype=dtype)[0].sqrt()
        return y.view(B, T, Wo, Cout), y_norm.view(B, T, Wo, Cout), dx, dx_norm

    (y64, yn, dx64, dxn), (y32, _, dx32, _) = ref(D), ref(F32)
    xd, wd, bd = dev(x).requires_grad_(), dev(w).requires_grad_(), dev(b).requires_grad_()
    y = ops.conv2d_3x3s2(xd, wd, bd)
    y.backward(dev(dy))
    check_scaled("conv2d_3x3s2 y [2, 2, 4, 32 -> 32]", y, y64, y32, yn)
    check_scaled("conv2d_3x3s2 dx [2, 2, 4, 32 -> 32]", xd.grad, dx64, dx32, dxn)
    check_scaled("conv2d_3x3s2 dx last column [2, 2, 4, 32 -> 32]", xd.grad[:, :, W - 1], dx64[:, :, W - 1], dx32[:, :, W - 1], dxn[:, :, W - 1])
