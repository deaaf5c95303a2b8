"""GPU: the kernels downstream of the model outputs in a train step - the eight variance / duration terms, BinLoss, the masked mean,
the mel L1 pair (csrc/loss.hip, csrc/optim.hip), the aligner's distance map and the ForwardSum CTC recursion (csrc/align.hip) and the
fused clip + Adam update (csrc/optim.hip) - term by term against the float64 restatement tests/loss_restate64.py, at the sizes where
their loops, caps and tails change behaviour and at the exact boundaries of their clamps.

Bars (all against float64): loss values 1e-5 relative, gradients 1e-5 of the tensor's largest magnitude, ForwardSum value and gradient
2e-5 (of max(1, largest magnitude), as tests/test_kernels_gpu.py), Adam parameters 2e-6 * max(1, |p|) per step, gradient norm 1e-5
relative.  Every comparison also evaluates the same formula with stock torch in float32 on the CPU and prints both errors (run with
-s to see them): a kernel that misses a bar which stock float32 meets with a wide margin has a precision bug."""
import pytest
import torch

import ctts_amd  # noqa: F401
from ctts_amd import _lib
from ctts_amd import kernels as K
from ctts_amd import ops
from ctts_amd._lib import CttsError
from tests import loss_restate64 as L64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIL = (357, 358, 359)                       # "@sp", "@spn", "@sil": the silence tokens that delimit words
SIL_T = torch.tensor(SIL, dtype=torch.int64)
VAL_TOL, GRAD_TOL, FS_TOL, ADAM_TOL, NORM_TOL = 1e-5, 1e-5, 2e-5, 2e-6, 1e-5
SRC_LENS = [300, 257, 256, 255, 1, 2, 64, 65, 128, 200, 17, 33, 299, 100, 150, 3]
MEL_LENS = [1024, 1, 1000, 513, 512, 511, 257, 256, 255, 64, 2, 777, 900, 128, 300, 1023]
LAMBDAS = (0.7, 1.3, 0.9, 1.1, 0.6)         # ph, word, sent, f0, uv: distinct, so a term scaled by another's lambda shows
W_A = (0.9, -1.3, 0.0, 2.1, 0.6, 1.7, -0.4, 1.2)       # upstream gradients of the eight terms: distinct, one zero, negatives
W_B = (-0.8, 0.5, 1.9, 0.0, 1.4, -2.2, 0.3, 0.7)
W_C = (1.1, 0.8, -1.6, 0.7, 0.0, 2.3, -0.5, 0.9)
PRED = ("log_d", "cwt", "f0m", "f0s", "e_pred")          # the five tensors that receive a gradient


def leaf(t, dtype, grad=True):
    """a fresh CPU leaf of `t` in `dtype`"""
    return t.detach().to(dtype).clone().requires_grad_(grad)


def _rel(got, ref):
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1e-30)


def check_values(name, got, ref64, ref32, tol=VAL_TOL, names=None):
    """|got - ref64| <= tol * |ref64| per element; a reference of exactly 0 must be met exactly"""
    got, ref64, ref32 = [t.detach().double().cpu().reshape(-1) for t in (got, ref64, ref32)]
    for i in range(ref64.numel()):
        n = f"{name}[{names[i] if names else i}]"
        if float(ref64[i]) == 0.0:
            print(f"{n}: reference 0, kernel {float(got[i])!r}")
            assert float(got[i]) == 0.0, n
            continue
        e, e32 = _rel(got[i], ref64[i]), _rel(ref32[i], ref64[i])
        print(f"{n}: kernel rel err {e:.2e}  stock float32 {e32:.2e}  bar {tol:.0e}")
        assert e <= tol, f"{n}: {float(got[i])!r} vs {float(ref64[i])!r} (rel {e:.3e} > {tol})"


def check_grad(name, got, ref64, ref32, tol=GRAD_TOL, floor=0.0):
    """max |got - ref64| <= tol * max(floor, max |ref64|)"""
    got, ref64, ref32 = [t.detach().double().cpu() for t in (got, ref64, ref32)]
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    scale = max(floor, ref64.abs().max().item()) if ref64.numel() else 1.0
    if scale == 0.0:
        print(f"{name}: reference all 0")
        assert got.abs().max().item() == 0.0, name
        return
    e, e32 = (got - ref64).abs().max().item() / scale, (ref32 - ref64).abs().max().item() / scale
    print(f"{name}: kernel err / max {e:.2e}  stock float32 {e32:.2e}  bar {tol:.0e}  (max {scale:.3e})")
    assert torch.isfinite(got).all(), name
    assert e <= tol, f"{name}: err / max {e:.3e} > {tol}"


# ------------------------------------------------------------------------------------------------ variance / duration terms
def var_batch(src_lens, mel_lens, Ts, Tm, seed, p_sil=0.15, dur_float=False):
    """CPU tensors in the layout of a collated batch: pads hold token 0, duration 0, log_d 0 (what the model's masked_fill leaves)"""
    g = torch.Generator().manual_seed(seed)
    B = len(src_lens)
    src_pad = torch.arange(Ts)[None, :] >= torch.tensor(src_lens)[:, None]
    mel_pad = torch.arange(Tm)[None, :] >= torch.tensor(mel_lens)[:, None]
    texts = torch.randint(1, 357, (B, Ts), generator=g)
    sil = torch.rand(B, Ts, generator=g) < p_sil
    texts = torch.where(sil, torch.tensor(SIL)[torch.randint(0, 3, (B, Ts), generator=g)], texts).masked_fill(src_pad, 0)
    dur = torch.randint(0, 9, (B, Ts), generator=g).masked_fill(src_pad, 0)
    log_d = (torch.randn(B, Ts, generator=g) * 0.7 + 1.0).masked_fill(src_pad, 0.0)
    return dict(log_d=log_d, cwt=torch.randn(B, Tm, 11, generator=g), f0m=torch.randn(B, generator=g), f0s=torch.randn(B, generator=g),
                e_pred=torch.randn(B, Ts, generator=g), dur=dur.float() if dur_float else dur, texts=texts, src_pad=src_pad,
                cwt_spec=torch.randn(B, Tm, 10, generator=g), uv=(torch.rand(B, Tm, generator=g) < 0.4).float(), mel_pad=mel_pad,
                f0m_t=torch.randn(B, generator=g), f0s_t=torch.randn(B, generator=g), e_tgt=torch.randn(B, Ts, generator=g))


ORDER = ("log_d", "cwt", "f0m", "f0s", "e_pred", "dur", "texts", "src_pad", "cwt_spec", "uv", "mel_pad", "f0m_t", "f0s_t", "e_tgt")


def var_kernel(b, lambdas=LAMBDAS, cwt_l2=0, w=W_A, grads=True):
    """ops.variance_losses with (terms * w).sum().backward(), run twice: -> (terms, {name: gradient}) on the CPU, bit-identical runs"""
    lam_t = torch.tensor(lambdas, dtype=torch.float32)
    runs = []
    for _ in range(2):
        d = {k: v.detach().to(DEV) for k, v in b.items()}
        for k in PRED:
            d[k] = d[k].clone().requires_grad_(grads)
        terms = ops.variance_losses(*[d[k] for k in ORDER], lam_t, cwt_l2, SIL_T)
        gr = {}
        if grads:
            (terms * torch.tensor(w, device=DEV)).sum().backward()
            gr = {k: d[k].grad.cpu() for k in PRED}
        runs.append((terms.detach().cpu(), gr))
    assert torch.equal(torch.nan_to_num(runs[0][0], nan=-7.0), torch.nan_to_num(runs[1][0], nan=-7.0))
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), f"d {k} differs between two runs"
    return runs[0]


def var_ref(b, lambdas=LAMBDAS, cwt_l2=0, w=W_A, dtype=torch.float64, grads=True):
    d = dict(b)
    for k in PRED:
        d[k] = leaf(b[k], dtype, grads)
    terms = L64.variance_terms(*[d[k] for k in ORDER], lambdas, cwt_l2, SIL, dtype=dtype)
    gr = {}
    if grads:
        (terms * torch.tensor(w, dtype=dtype)).sum().backward()
        gr = {k: d[k].grad for k in PRED}
    return terms.detach(), gr


def var_compare(name, b, lambdas=LAMBDAS, cwt_l2=0, w=W_A):
    terms, gr = var_kernel(b, lambdas, cwt_l2, w)
    t64, g64 = var_ref(b, lambdas, cwt_l2, w)
    t32, g32 = var_ref(b, lambdas, cwt_l2, w, dtype=torch.float32)
    assert float(t64[1]) == float(t64[1]) and ((~b["src_pad"]).sum() > 0), "this helper is for batches with sum wn > 0 and sum nonpad > 0"
    check_values(name, terms, t64, t32, names=L64.TERMS)
    for k in PRED:
        check_grad(f"{name} d {k}", gr[k], g64[k], g32[k])
    return terms, gr, t64, g64


@pytest.mark.parametrize("w", [W_A, W_B], ids=["wA", "wB"])
@pytest.mark.parametrize("cwt_l2", [0, 1])
@pytest.mark.parametrize("dur_float", [False, True], ids=["dur_int64", "dur_float32"])
def test_variance_terms_ragged_batch_of_16(dur_float, cwt_l2, w):
    """B = 16, Ts = 300 (second stride iteration of the token loops), Tm = 1024, ragged lengths incl. 1 and the full width: all eight
    values and all five gradients under eight distinct upstream weights.  Stock float32 measured on this batch: values 1-5e-8,
    gradients about 1e-7 of the maximum."""
    b = var_batch(SRC_LENS, MEL_LENS, 300, 1024, seed=1, dur_float=dur_float)
    assert b["dur"].dtype == (torch.float32 if dur_float else torch.int64)
    var_compare("ragged16", b, cwt_l2=cwt_l2, w=w)


@pytest.mark.parametrize("Ts,Tm,sl,ml", [(37, 50, 37, 50), (300, 1024, 280, 1000), (1, 1, 1, 1)])
def test_variance_terms_single_utterance(Ts, Tm, sl, ml):
    b = var_batch([sl], [ml], Ts, Tm, seed=2)
    if Ts == 1:                                   # a single token forms no word (0/0): the word term is switched off
        var_compare("B1 one token", b, lambdas=(0.7, 0.0, 0.9, 1.1, 0.6))
        return
    b["texts"][0, 3] = SIL[0]
    b["dur"][0, 4] = 3                            # a word with a positive target behind a silence: sum wn > 0
    var_compare("B1", b)


@pytest.mark.parametrize("off", ["word", "sent"])
def test_variance_terms_switched_off_term_is_exactly_zero_and_the_rest_unchanged(off):
    b = var_batch(SRC_LENS, MEL_LENS, 300, 1024, seed=3)
    full, _ = var_kernel(b, grads=False)
    lam = list(LAMBDAS)
    idx = {"word": 1, "sent": 2}[off]
    lam[idx] = 0.0
    terms, gr, t64, g64 = var_compare(f"lambda_{off} = 0", b, lambdas=tuple(lam), w=W_B)
    assert float(terms[idx]) == 0.0 and float(t64[idx]) == 0.0
    keep = [i for i in range(8) if i != idx]
    assert terms[keep].tolist() == full[keep].tolist()


def word_case(rows, durs, pad_to, log_d_pad=0.0, seed=4):
    """batch from explicit token rows (lists of ids; 's' = a silence token) and target durations, padded with token 0 to `pad_to`"""
    B = len(rows)
    lens = [len(r) for r in rows]
    b = var_batch(lens, [20] * B, pad_to, 20, seed=seed)
    for i, (r, d) in enumerate(zip(rows, durs)):
        assert len(r) == len(d)
        b["texts"][i, :len(r)] = torch.tensor([SIL[j % 3] if t == "s" else t for j, t in enumerate(r)])
        b["dur"][i, :len(d)] = torch.tensor(d)
    b["log_d"] = b["log_d"].masked_fill(b["src_pad"], log_d_pad)
    return b


ONLY_WDUR = (0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
NORMAL = (["s", 11, 12, "s", 13, 14, 15], [1, 2, 3, 1, 4, 0, 2])         # keeps sum wn > 0 in every word-edge batch


def _word_edge(name, b, zero_tokens=(), nonzero_tokens=()):
    """full comparison, then a run whose only upstream weight is wdur's: tokens outside every counted word get exactly no gradient"""
    var_compare(name, b)
    var_compare(name + " l2", b, cwt_l2=1, w=W_B)
    _, gr = var_kernel(b, w=ONLY_WDUR)
    _, g64 = var_ref(b, w=ONLY_WDUR)
    for (i, t) in zero_tokens:
        assert float(g64["log_d"][i, t]) == 0.0 and float(gr["log_d"][i, t]) == 0.0, (name, i, t, float(gr["log_d"][i, t]))
    for (i, t) in nonzero_tokens:
        assert float(g64["log_d"][i, t]) != 0.0 and float(gr["log_d"][i, t]) != 0.0, (name, i, t)
    check_grad(name + " d log_d (wdur only)", gr["log_d"], g64["log_d"], var_ref(b, w=ONLY_WDUR, dtype=torch.float32)[1]["log_d"])


def test_word_edge_leading_tokens_before_the_first_silence_belong_to_no_word():
    b = word_case([[21, 22, 23, "s", 24, 25, "s", 26], NORMAL[0]], [[3, 2, 5, 1, 2, 2, 0, 4], NORMAL[1]], 8)
    assert L64.word_ids(b["texts"], SIL)[0].tolist() == [0, 0, 0, 0, 1, 1, 0, 2]
    _word_edge("leading tokens", b, zero_tokens=[(0, 0), (0, 1), (0, 2), (0, 3), (0, 6)], nonzero_tokens=[(0, 4), (0, 5), (0, 7)])


def test_word_edge_consecutive_silences_leave_empty_word_ids():
    b = word_case([["s", 21, 22, "s", "s", "s", 23, 24], NORMAL[0]], [[2, 2, 1, 3, 1, 1, 2, 5], NORMAL[1]], 8)
    assert L64.word_ids(b["texts"], SIL)[0].tolist() == [0, 1, 1, 0, 0, 0, 4, 4]
    _word_edge("consecutive silences", b, zero_tokens=[(0, 0), (0, 3), (0, 4), (0, 5)], nonzero_tokens=[(0, 1), (0, 2), (0, 6), (0, 7)])


def test_word_edge_a_word_whose_target_durations_are_all_zero_is_not_counted():
    b = word_case([["s", 21, 22, "s", 23, 24, "s", 25], NORMAL[0]], [[1, 2, 1, 1, 0, 0, 2, 3], NORMAL[1]], 8)
    t, _ = var_ref(b)
    _word_edge("all-zero word", b, zero_tokens=[(0, 4), (0, 5)], nonzero_tokens=[(0, 1), (0, 2), (0, 7)])
    b2 = {k: v.clone() for k, v in b.items()}
    b2["log_d"][0, 4:6] += 1.0                    # the uncounted word's prediction does not enter wdur (it does enter sdur)
    t2, _ = var_ref(b2)
    k1, k2 = var_kernel(b, grads=False)[0], var_kernel(b2, grads=False)[0]
    assert float(t[1]) == float(t2[1]) and float(k1[1]) == float(k2[1]) and float(k1[2]) != float(k2[2])


def test_word_edge_an_utterance_without_a_silence_contributes_no_word():
    b = word_case([[21, 22, 23, 24, 25, 26], NORMAL[0]], [[3, 2, 5, 1, 2, 2], NORMAL[1]], 7)
    assert L64.word_ids(b["texts"], SIL)[0].tolist() == [0] * 7
    _word_edge("no silence", b, zero_tokens=[(0, t) for t in range(7)], nonzero_tokens=[(1, 1), (1, 2)])


@pytest.mark.parametrize("log_d_pad", [0.0, 0.3])
def test_word_edge_pad_tokens_join_the_last_word(log_d_pad):
    """pads carry token 0, which is no silence: they extend the last word.  With log_d == 0 there (the model's masked_fill) their linear
    duration is 0 but the clamp's slope at its bound is 1, as autograd's; with garbage 0.3 they also move the word's sum."""
    b = word_case([["s", 21, 22], NORMAL[0]], [[1, 2, 4], NORMAL[1]], 12, log_d_pad=log_d_pad)
    assert L64.word_ids(b["texts"], SIL)[0].tolist() == [0, 1, 1] + [1] * 9
    _word_edge("pads join", b, zero_tokens=[(0, 0)], nonzero_tokens=[(0, 1), (0, 2)] + [(0, t) for t in range(3, 12)])


def test_word_edge_an_utterance_made_only_of_silences():
    b = word_case([["s", "s", "s", "s"], NORMAL[0]], [[2, 1, 3, 1], NORMAL[1]], 7)
    assert L64.word_ids(b["texts"], SIL)[0, :4].tolist() == [0, 0, 0, 0]
    _word_edge("only silences", b, zero_tokens=[(0, t) for t in range(4)], nonzero_tokens=[(1, 1)])


@pytest.mark.parametrize("cwt_l2", [0, 1])
def test_variance_terms_exact_boundaries_follow_autograd(cwt_l2):
    """log_d == 0 at valid tokens and at every pad (slope of clamp(exp(x) - 1, min 0) at its bound: 1, as torch's clamp), cwt == cwt_spec,
    e_pred == e_tgt and equal f0 statistics (slope of |x| at 0: exactly 0)."""
    b = var_batch(SRC_LENS, MEL_LENS, 300, 1024, seed=5)
    valid0 = (torch.rand(16, 300, generator=torch.Generator().manual_seed(6)) < 0.2) & ~b["src_pad"]
    b["log_d"][valid0] = 0.0
    eq_c = torch.rand(16, 1024, 10, generator=torch.Generator().manual_seed(7)) < 0.3
    b["cwt"][:, :, :10][eq_c] = b["cwt_spec"][eq_c]
    eq_e = torch.rand(16, 300, generator=torch.Generator().manual_seed(8)) < 0.3
    b["e_pred"][eq_e] = b["e_tgt"][eq_e]
    b["f0m"][::3] = b["f0m_t"][::3]
    b["f0s"][1::4] = b["f0s_t"][1::4]
    assert float(b["log_d"][b["src_pad"]].abs().max()) == 0.0 and int(valid0.sum()) > 100
    _, gr, _, g64 = var_compare("boundaries", b, cwt_l2=cwt_l2, w=W_C)
    for k in ("cwt", "e_pred", "f0m", "f0s"):     # sign at 0 and the zeros outside the limits: exactly torch's
        z = g64[k] == 0
        assert int(z.sum()) > 0 and float(gr[k][z].abs().max()) == 0.0, k
        assert torch.equal(gr[k] == 0, z), k
    at0 = (b["log_d"] == 0)
    assert float(g64["log_d"][at0].abs().min()) > 0.0           # autograd passes the clamp's gradient at the bound ...
    assert torch.equal(gr["log_d"] == 0, g64["log_d"] == 0)     # ... and so does the kernel, at valid tokens and at pads


def test_variance_terms_ignore_garbage_at_padded_positions():
    """garbage at the pads of dur, e_pred and the uv logit moves nothing; garbage at the pads of log_d moves only wdur and sdur (the
    reference sums the linear durations over pads too); the C term includes padded frames by design."""
    b = var_batch(SRC_LENS, MEL_LENS, 300, 1024, seed=9)
    clean, gclean = var_kernel(b)
    g = torch.Generator().manual_seed(10)
    b1 = {k: v.clone() for k, v in b.items()}
    b1["dur"][b["src_pad"]] = torch.randint(1, 50, (int(b["src_pad"].sum()),), generator=g)
    b1["e_pred"][b["src_pad"]] = torch.randn(int(b["src_pad"].sum()), generator=g) * 30
    b1["cwt"][:, :, 10][b["mel_pad"]] = torch.randn(int(b["mel_pad"].sum()), generator=g) * 30
    t1, g1, _, _ = var_compare("garbage dur/e/uv", b1)
    assert t1.tolist() == clean.tolist()
    assert float(g1["e_pred"][b["src_pad"]].abs().max()) == 0.0 and float(g1["cwt"][:, :, 10][b["mel_pad"]].abs().max()) == 0.0
    assert torch.equal(g1["log_d"], gclean["log_d"]) and torch.equal(g1["cwt"][:, :, :10], gclean["cwt"][:, :, :10])
    b2 = {k: v.clone() for k, v in b1.items()}
    b2["log_d"][b["src_pad"]] = torch.randn(int(b["src_pad"].sum()), generator=g)
    t2, _, _, _ = var_compare("garbage log_d", b2)
    for i in (0, 3, 4, 5, 6, 7):
        assert float(t2[i]) == float(clean[i]), L64.TERMS[i]
    assert float(t2[1]) != float(clean[1]) and float(t2[2]) != float(clean[2])
    cpad = {k: v.clone() for k, v in b.items()}
    cpad["cwt_spec"][b["mel_pad"]] += 1.0           # padded frames count in C
    assert float(var_kernel(cpad, grads=False)[0][3]) != float(clean[3])


def test_variance_terms_batch_without_any_silence_gives_nan_wdur_as_the_reference():
    """0 words: wdur = 0/0 = NaN in the reference and here; the other seven terms are those of the same batch with the word term
    switched off.  The word term then sends NO gradient (include/ctts.h): no token belongs to a counted word, so every gradient is
    finite, is autograd's, and equals bit for bit that of the same batch with lambda_word = 0 - the NaN stays in the value."""
    b = var_batch(SRC_LENS, MEL_LENS, 300, 1024, seed=11, p_sil=0.0)
    terms, gr = var_kernel(b)
    t64, g64 = var_ref(b)
    t32, g32 = var_ref(b, dtype=torch.float32)
    assert torch.isnan(t64[1]) and torch.isnan(terms[1])
    off, groff = var_kernel(b, lambdas=(0.7, 0.0, 0.9, 1.1, 0.6))
    for k in PRED:
        assert torch.isfinite(g64[k]).all() and torch.isfinite(gr[k]).all(), k
        assert torch.equal(gr[k], groff[k]), f"d {k}: the word term of a batch without words must send no gradient"
        check_grad(f"no silence in the batch d {k}", gr[k], g64[k], g32[k])
    keep = [0, 2, 3, 4, 5, 6, 7]
    assert terms[keep].tolist() == off[keep].tolist()
    check_values("no silence in the batch", terms[keep], t64[keep], t32[keep], names=[L64.TERMS[i] for i in keep])


# ------------------------------------------------------------------------------------------------ BinLoss
def bin_compare(name, hard, soft, w=-1.7, ordinary=None):
    runs = []
    for _ in range(2):
        s = soft.to(DEV).clone().requires_grad_(True)
        v = ops.bin_loss(hard.to(DEV), s)
        (v * w).backward()
        runs.append((v.detach().cpu(), s.grad.cpu()))
    assert float(runs[0][0]) == float(runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ref = {}
    for dt in (torch.float64, torch.float32):
        s = leaf(soft, dt)
        v = L64.bin_loss(hard, s, dtype=dt)
        (v * w).backward()
        ref[dt] = (v.detach(), s.grad)
    check_values(name, runs[0][0], ref[torch.float64][0], ref[torch.float32][0])
    check_grad(name + " d soft", runs[0][1], ref[torch.float64][1], ref[torch.float32][1])
    if ordinary is not None:      # the gradient at the bound is 1e12 / sum(hard): compare the ordinary elements on their own scale too
        check_grad(name + " d soft (soft > 1e-6)", runs[0][1][ordinary], ref[torch.float64][1][ordinary], ref[torch.float32][1][ordinary])
    g, g64, g32 = runs[0][1].double(), ref[torch.float64][1], ref[torch.float32][1].double()
    nz = g64 != 0                 # element by element: -w * hard / (soft * sum hard) is one product, nothing cancels
    assert torch.equal(g != 0, nz)
    e, e32 = ((g - g64).abs()[nz] / g64.abs()[nz]).max().item(), ((g32 - g64).abs()[nz] / g64.abs()[nz]).max().item()
    print(f"{name} d soft, element-wise relative: kernel {e:.2e}  stock float32 {e32:.2e}  bar {GRAD_TOL:.0e}")
    assert e <= GRAD_TOL, f"{name}: element-wise relative gradient error {e:.3e}"
    return runs[0], ref[torch.float64]


def test_bin_loss_full_size_one_hot_ragged_with_values_at_and_below_the_clamp():
    """n = 16 * 1024 * 150 (grid capped at 512 blocks, grid-stride loop), hard = one token per valid frame, soft containing 0, 1e-13,
    exactly the bound 1e-12 and 1 at selected and at unselected positions.  At the bound the gradient passes (1 / soft), below it is 0."""
    B, Tm, Ts = 16, 1024, 150
    g = torch.Generator().manual_seed(12)
    klens = [min(l, Ts) for l in SRC_LENS]
    soft = torch.softmax(torch.randn(B, Tm, Ts, generator=g) * 3, dim=-1)
    hard = torch.zeros(B, Tm, Ts)
    for b in range(B):
        idx = torch.randint(0, klens[b], (MEL_LENS[b],), generator=g)
        hard[b, torch.arange(MEL_LENS[b]), idx] = 1.0
    sel = hard.nonzero()
    bound = torch.tensor(1e-12, dtype=torch.float32)
    specials = [0.0, 1e-13, float(bound), 1.0]
    for j, val in enumerate(specials * 3):
        bb, t, k = sel[37 * j + 5].tolist()
        soft[bb, t, k] = val                                     # where hard == 1
        soft[bb, t, (k + 1) % Ts] = val                          # and next to it, where hard == 0
    assert int((soft == bound).sum()) >= 3 and int((soft == 0).sum()) >= 3 and float(hard.sum()) == sum(MEL_LENS)
    (v, gs), (v64, g64) = bin_compare("bin full", hard, soft, ordinary=soft > 1e-6)
    at = (soft == bound) & (hard == 1)
    below = (soft < bound)
    assert float(g64[at].abs().min()) > 0 and float(gs[at].abs().min()) > 0         # the bound passes the gradient, as torch's clamp
    assert float(g64[below].abs().max()) == 0.0 and float(gs[below].abs().max()) == 0.0
    assert torch.equal(gs == 0, g64 == 0)


@pytest.mark.parametrize("n", [1, 131071, 131072, 131073])
def test_bin_loss_sizes_around_the_block_cap(n):
    g = torch.Generator().manual_seed(n)
    soft = torch.rand(n, generator=g).clamp(min=1e-4)
    hard = (torch.rand(n, generator=g) < 0.3).float()
    hard[0] = 1.0
    bin_compare(f"bin n={n}", hard, soft)


# ------------------------------------------------------------------------------------------------ masked mean
def masked_compare(name, p, t, w, kind, up=3.0):
    runs = []
    for _ in range(2):
        pd = p.to(DEV).clone().requires_grad_(True)
        v = ops.masked_loss(pd, t.to(DEV), w.to(DEV), kind)
        (v * up).backward()
        runs.append((v.detach().cpu(), pd.grad.cpu()))
    assert float(runs[0][0]) == float(runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ref = {}
    for dt in (torch.float64, torch.float32):
        pp = leaf(p, dt)
        v = L64.masked_mean(pp, t, w, kind, dtype=dt)
        (v * up).backward()
        ref[dt] = (v.detach(), pp.grad)
    check_values(name, runs[0][0], ref[torch.float64][0], ref[torch.float32][0])
    check_grad(name + " d pred", runs[0][1], ref[torch.float64][1], ref[torch.float32][1])
    return runs[0], ref[torch.float64]


@pytest.mark.parametrize("kind", ["l1", "l2", "bce"])
@pytest.mark.parametrize("n", [16000, 131071, 131072, 131073])
def test_masked_loss_sizes_around_the_block_cap(n, kind):
    g = torch.Generator().manual_seed(17 + n)
    p = torch.randn(n, generator=g)
    t = (torch.rand(n, generator=g) < 0.4).float() if kind == "bce" else torch.randn(n, generator=g)
    w = (torch.rand(n, generator=g) < 0.7).float()
    p[::5] = t[::5]                                              # |x| at 0: slope exactly 0
    (_, gp), (_, g64) = masked_compare(f"masked {kind} n={n}", p, t, w, kind)
    assert torch.equal(gp == 0, g64 == 0)


@pytest.mark.parametrize("kind", ["l1", "l2", "bce"])
def test_masked_loss_weight_vector_with_a_single_non_zero(kind):
    n = 70001
    g = torch.Generator().manual_seed(18)
    p, w = torch.randn(n, generator=g), torch.zeros(n)
    t = (torch.rand(n, generator=g) < 0.4).float() if kind == "bce" else torch.randn(n, generator=g)
    w[54321] = 2.5
    (_, gp), _ = masked_compare(f"masked {kind} one weight", p, t, w, kind)
    assert int((gp != 0).sum()) == 1 and float(gp[54321]) != 0.0


# ------------------------------------------------------------------------------------------------ mel L1 pair
def mel_l1_abi(p1, p2, tgt, pad, use_ws, rows=None):
    """ctts_mel_l1_fwd through the C ABI with NaN-filled outputs -> (sums [3], roww)"""
    Cc = tgt.shape[-1]
    rows = tgt.numel() // Cc if rows is None else rows
    sums = torch.full((3,), float("nan"), device=DEV)
    roww = torch.full((max(rows, 1),), float("nan"), device=DEV)
    ws = K._ws(tgt) if use_ws else None
    _lib.check(_lib.load().ctts_mel_l1_fwd(K._p(p1), K._p(p2), K._p(tgt), K._p(pad), K._p(sums), K._p(roww), rows, Cc, ws, K._stream()),
               "ctts_mel_l1_fwd")
    torch.cuda.synchronize()
    return sums.cpu(), roww.cpu()


def _mel_batch(B, T, Cc, lens, seed):
    g = torch.Generator().manual_seed(seed)
    tgt = torch.randn(B, T, Cc, generator=g)
    tgt[0, 5] = 0.0                                             # an all-zero target row inside the valid region: weight 0
    pad = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
    return torch.randn(B, T, Cc, generator=g), torch.randn(B, T, Cc, generator=g), tgt, pad


def test_mel_l1_writes_its_sums_on_both_reduction_paths():
    """sums arrives NaN-filled: the kernel writes it (it does not accumulate), on the one-workgroup path (ws NULL) and on the ordered
    multi-workgroup path (525 workgroups, two-level sum); both against float64, each bit-identical when repeated."""
    B, T, Cc = 3, 700, 80
    p1, p2, tgt, pad = _mel_batch(B, T, Cc, [700, 333, 1], 19)
    d = [x.to(DEV) for x in (p1, p2, tgt)] + [pad.to(DEV).view(torch.uint8)]
    losses64, sums64, w64 = L64.mel_l1_pair(p1, p2, tgt, pad)
    _, sums32, _ = L64.mel_l1_pair(p1, p2, tgt, pad, dtype=torch.float32)
    for use_ws in (False, True):
        s, roww = mel_l1_abi(*d, use_ws)
        s2, roww2 = mel_l1_abi(*d, use_ws)
        assert torch.equal(s, s2) and torch.equal(roww, roww2)
        assert torch.equal(roww.double(), w64.reshape(-1))
        check_values(f"mel l1 sums ws={use_ws}", s, sums64, sums32)
    assert float(sums64[2]) == 700 - 1 + 333 + 1


def test_mel_l1_zero_rows_writes_three_zeros():
    p1, p2, tgt, pad = _mel_batch(1, 8, 80, [8], 20)
    d = [x.to(DEV) for x in (p1, p2, tgt)] + [pad.to(DEV).view(torch.uint8)]
    for use_ws in (False, True):
        s, roww = mel_l1_abi(*d, use_ws, rows=0)
        assert s.tolist() == [0.0, 0.0, 0.0] and torch.isnan(roww).all()


def test_mel_l1_pair_values_and_gradients():
    B, T, Cc = 3, 700, 80
    p1, p2, tgt, pad = _mel_batch(B, T, Cc, [700, 333, 1], 21)
    p1[1, 7, :40] = tgt[1, 7, :40]                                # sign at 0
    up = torch.tensor([0.7, -1.3])
    runs = []
    for _ in range(2):
        a, b = p1.to(DEV).clone().requires_grad_(True), p2.to(DEV).clone().requires_grad_(True)
        both = ops.mel_l1_pair(a, b, tgt.to(DEV), pad.to(DEV))
        (both * up.to(DEV)).sum().backward()
        runs.append((both.detach().cpu(), a.grad.cpu(), b.grad.cpu()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    ref = {}
    for dt in (torch.float64, torch.float32):
        a, b = leaf(p1, dt), leaf(p2, dt)
        both = L64.mel_l1_pair(a, b, tgt, pad, dtype=dt)[0]
        (both * up.to(dt)).sum().backward()
        ref[dt] = (both.detach(), a.grad, b.grad)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    check_values("mel l1 pair", runs[0][0], r64[0], r32[0])
    check_grad("d mel", runs[0][1], r64[1], r32[1])
    check_grad("d postnet mel", runs[0][2], r64[2], r32[2])
    assert torch.equal(runs[0][1] == 0, r64[1] == 0) and torch.equal(runs[0][2] == 0, r64[2] == 0)


# ------------------------------------------------------------------------------------------------ -temp * ||q - k||^2
def sqdist_abi(q, k, temp):
    B, Tq, Cc = q.shape
    Tk = k.shape[1]
    out = torch.full((B, Tq, Tk), float("nan"), device=DEV)
    _lib.check(_lib.load().ctts_neg_sqdist(K._p(q), K._p(k), K._p(out), B, Tq, Tk, Cc, float(temp), K._stream()), "ctts_neg_sqdist")
    return out


@pytest.mark.parametrize("B,Tq,Tk,Cc", [(3, 130, 70, 80), (1, 1, 1, 80), (2, 64, 64, 80), (2, 1024, 150, 80), (2, 70, 130, 1), (1, 65, 129, 255)])
def test_neg_sqdist_against_float64(B, Tq, Tk, Cc):
    """Every element of a NaN-filled output is written, tile edges in Tq / Tk included.  Bar, element by element: 1e-5 * |reference|
    for every shape (all C terms of a sum of squares are non-negative, so nothing cancels; stock float32 measured at 2-3e-7)."""
    g = torch.Generator().manual_seed(B * Tq + Tk + Cc)
    q, k = torch.randn(B, Tq, Cc, generator=g), torch.randn(B, Tk, Cc, generator=g)
    temp = 0.0005
    tol = VAL_TOL
    qd, kd = q.to(DEV), k.to(DEV)
    out = sqdist_abi(qd, kd, temp)
    assert torch.equal(out, sqdist_abi(qd, kd, temp)) and torch.equal(out, K.neg_sqdist(qd, kd, temp))
    out = out.cpu().double()
    assert torch.isfinite(out).all(), "unwritten (NaN) elements"
    worst = worst32 = 0.0
    for b in range(B):
        r64 = L64.neg_sqdist(q[b:b + 1], k[b:b + 1], temp)[0]
        r32 = L64.neg_sqdist(q[b:b + 1], k[b:b + 1], temp, dtype=torch.float32)[0].double()
        assert float(r64.max()) < 0.0
        worst = max(worst, ((out[b] - r64).abs() / r64.abs()).max().item())
        worst32 = max(worst32, ((r32 - r64).abs() / r64.abs()).max().item())
    print(f"neg_sqdist {B, Tq, Tk, Cc}: kernel rel err {worst:.2e}  stock float32 {worst32:.2e}  bar {tol:.1e}")
    assert worst <= tol


def test_neg_sqdist_refuses_256_channels():
    q, k = torch.zeros(1, 4, 256, device=DEV), torch.zeros(1, 4, 256, device=DEV)
    with pytest.raises(CttsError, match="C too large for the LDS tile"):
        K.neg_sqdist(q, k, 0.0005)
    assert float(K.neg_sqdist(q[:, :, :255].contiguous(), k[:, :, :255].contiguous(), 1.0).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ ForwardSum (CTC)
def fs_inputs(B, Tm, Ts, seed):
    return torch.randn(B, Tm, Ts, generator=torch.Generator().manual_seed(seed)) * 2


def fs_weights(B):
    return torch.tensor([(0.5 + 0.1 * b) * (-1) ** b for b in range(B)])


def fs_ref(a, in_lens, out_lens, dtype):
    x = leaf(a, dtype)
    nll, nll0 = L64.forward_sum_nll(x, in_lens, out_lens, -1.0, dtype=dtype)
    (nll0 * fs_weights(a.shape[0]).to(dtype)).sum().backward()
    return nll.detach(), x.grad


def fs_compare(name, a, in_lens, out_lens, grad_f32=0.0):
    """`grad_f32`: the error of stock float32 CTC's gradient measured on this case.  Where it exceeds a quarter of the 2e-5 bar the
    gradient bar is 4 times that measurement (float32 log-space arithmetic at |alpha + beta| of several thousand cannot do better; the
    factor 4 covers an equivalent, differently ordered evaluation).  The bar of the VALUE stays 2e-5 in every case."""
    B = a.shape[0]
    grad_tol = FS_TOL if grad_f32 <= FS_TOL / 4 else 4 * grad_f32
    il, ol = torch.tensor(in_lens), torch.tensor(out_lens)
    runs = []
    for _ in range(2):
        ad = a.to(DEV).clone().requires_grad_(True)
        nll = ops.forward_sum_nll(ad, il.to(DEV), ol.to(DEV), -1.0)
        nll0 = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)              # zero_infinity, as the loss does
        (nll0 * fs_weights(B).to(DEV)).sum().backward()
        runs.append((nll.detach().cpu(), ad.grad.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    nll, grad = runs[0]
    n64, g64 = fs_ref(a, in_lens, out_lens, torch.float64)
    n32, g32 = fs_ref(a, in_lens, out_lens, torch.float32)
    inf = torch.isinf(n64)
    assert torch.equal(torch.isinf(nll), inf) and (nll[inf] > 0).all(), (nll, n64)
    for b in range(B):
        if inf[b]:
            assert in_lens[b] > out_lens[b]
            assert float(grad[b].abs().max()) == 0.0, f"{name}: gradient of an infinite nll must be zero"
            continue
        e = abs(float(nll[b]) - float(n64[b])) / max(1.0, abs(float(n64[b])))
        e32 = abs(float(n32[b]) - float(n64[b])) / max(1.0, abs(float(n64[b])))
        print(f"{name} nll[{b}] (K={in_lens[b]}, T={out_lens[b]}) = {float(n64[b]):.4f}: kernel err {e:.2e}  stock float32 {e32:.2e}  bar {FS_TOL:.0e}")
        assert e <= FS_TOL, (name, b, float(nll[b]), float(n64[b]))
    if grad_f32:                                                  # the figure the bar rests on still describes this case
        e32 = (g32.double() - g64).abs().max().item() / max(1.0, g64.abs().max().item())
        assert grad_f32 / 2 <= e32 <= 2 * grad_f32, f"{name}: stock float32 gradient error {e32:.3e}, bar built on {grad_f32:.3e}: re-measure"
    check_grad(name + " d attn_logprob", grad, g64, g32, tol=grad_tol, floor=1.0)
    for b in range(B):                                            # zeros outside the limits: exactly
        assert float(grad[b, out_lens[b]:].abs().max() if out_lens[b] < a.shape[1] else 0.0) == 0.0
        assert float(grad[b, :, in_lens[b]:].abs().max() if in_lens[b] < a.shape[2] else 0.0) == 0.0
    return nll, grad


@pytest.mark.parametrize("B,Tm,Ts,in_lens,out_lens,grad_f32", [
    (2, 1100, 512, [512, 500], [1100, 1001], 2.88e-3),
    (2, 2100, 600, [600, 513], [2100, 1999], 1.37e-2),
    (1, 1030, 1023, [1023], [1030], 3.28e-3),
    (16, 1024, 160, [min(l, 160) for l in SRC_LENS], MEL_LENS, 3.11e-3),
], ids=["2x1100x512", "2x2100x600", "1x1030x1023", "16x1024x160"])
def test_forward_sum_long_recursions_and_two_states_per_thread(B, Tm, Ts, in_lens, out_lens, grad_f32):
    """Ts >= 512 launches the two-states-per-thread instantiation (512 <= Tk <= 1023); Tm up to 2100 runs the recursion twice as long as
    the train step does; the batch of 16 uses the ragged lengths of the other tests, several of them with more tokens than frames.

    Values: bar 2e-5 (stock float32 CTC measured at 2e-7 .. 5e-7 on these cases).  Gradients: stock float32 CTC on the CPU measured at
    2.88e-3 (2x1100x512), 1.37e-2 (2x2100x600), 3.28e-3 (1x1030x1023) and 3.11e-3 (16x1024x160) of max(1, largest magnitude) against
    float64 - the occupancies are exp() of sums of log-probabilities of magnitude 6,000 .. 14,000, whose float32 spacing is 5e-4 .. 1e-3.
    That is far above a quarter of the 2e-5 bar, so the gradient bars are 4 times these measurements: 1.15e-2, 5.5e-2, 1.31e-2, 1.24e-2."""
    fs_compare(f"forward-sum {B}x{Tm}x{Ts}", fs_inputs(B, Tm, Ts, seed=B + Tm + Ts), in_lens, out_lens, grad_f32)


def test_forward_sum_single_token_single_frame_and_more_tokens_than_frames():
    """(K, T) = (1, 30), (1, 1), (20, 20), (20, 10), (7, 1), (20, 30): K = 1, T = 1, T == K, and T < K (infinite nll: zero loss, zero
    gradient).  Stock float32 CTC's gradient measured at 9.70e-6 here (sums of magnitude 100, spacing 7.6e-6): more than a quarter of
    2e-5, so the gradient bar is 4 * 9.70e-6 = 3.9e-5; the value bar stays 2e-5."""
    ks, ts = [1, 1, 20, 20, 7, 20], [30, 1, 20, 10, 1, 30]
    nll, _ = fs_compare("forward-sum edges", fs_inputs(6, 30, 20, seed=23), ks, ts, grad_f32=9.70e-6)
    assert torch.isinf(nll).tolist() == [False, False, False, True, True, False]


def test_forward_sum_refuses_sizes_beyond_its_lds_rows():
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(CttsError, match="Tk <= 1023"):
        ops.forward_sum_nll(torch.zeros(1, 8, 1024, device=DEV), one, one)
    with pytest.raises(CttsError, match="beyond the LDS row buffers"):
        ops.forward_sum_nll(torch.zeros(1, 15000, 100, device=DEV), one, one)           # Tq + 2 (2 Tk + 1) floats > 60 KiB
    assert torch.isfinite(ops.forward_sum_nll(torch.zeros(1, 8, 1023, device=DEV), one, one)).all()


# ------------------------------------------------------------------------------------------------ clip + Adam
B1, B2, EPS = 0.9, 0.98, 1e-9


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def adam_run(n, wd, max_norm, start, steps, seed, check=True):
    """K.adam_clip_step on flat tensors, `steps` updates with the learning rate rewritten in its device scalar in between and the clip
    alternately active and idle; with `check`, each step against the float64 update (same float32-rounded scalars).  -> final state"""
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 0.1 if start else torch.zeros(n)            # a restored run brings its moments along
    v0 = torch.rand(n, generator=g) * 0.01 if start else torch.zeros(n)
    p64, m64, v64 = p0.double(), m0.double(), v0.double()
    p32, m32, v32 = p0.clone(), m0.clone(), v0.clone()                              # stock torch float32 on the CPU: the yardstick
    p, m, v = p0.clone().to(DEV), m0.clone().to(DEV), v0.clone().to(DEV)
    state = torch.zeros(_lib.ADAM_STATE_FLOATS, device=DEV)
    state[1] = float(start)
    lr = torch.zeros(1, device=DEV)
    for it in range(steps):
        lr.fill_(3e-3 * (1.0 + 0.5 * it))
        scale = (0.2 if it % 3 == 1 else 20.0) / max(1.0, n ** 0.5)               # norm about 0.2 (clip idle) or 20 (clip active)
        grad = torch.randn(n, generator=g) * scale
        K.adam_clip_step(p, grad.to(DEV), m, v, lr, B1, B2, EPS, wd, max_norm, state)
        if not check:
            continue
        total = L64.adam_clip_step(p64, grad.double(), m64, v64, start + it, float(lr.item()), _f32(B1), _f32(B2), _f32(EPS), _f32(wd),
                                   max_norm)
        total32 = L64.adam_clip_step(p32, grad, m32, v32, start + it, float(lr.item()), _f32(B1), _f32(B2), _f32(EPS), _f32(wd), max_norm)
        st = state[:3].cpu()
        e_n = _rel(st[2], total)
        scale = max(1.0, p64.abs().max().item())
        err, err32 = (p.cpu().double() - p64).abs().max().item() / scale, (p32.double() - p64).abs().max().item() / scale
        print(f"adam n={n} wd={wd} max_norm={max_norm} step {start + it + 1}: norm {float(total):.4f} kernel rel err {e_n:.2e}  stock float32 "
              f"{_rel(total32, total):.2e}  bar {NORM_TOL:.0e}; param err / max(1, |p|) kernel {err:.2e}  stock float32 {err32:.2e}  bar {ADAM_TOL:.0e}")
        assert e_n <= NORM_TOL and _rel(st[0], total ** 2) <= 2 * NORM_TOL       # state[2] reports the norm also when max_norm <= 0
        assert float(st[1]) == start + it + 1
        assert err <= ADAM_TOL, f"step {it}: {err:.3e}"
    return p.cpu(), m.cpu(), v.cpu(), state[:3].cpu()


@pytest.mark.parametrize("wd,max_norm,start", [(0.0, 1.0, 0), (1e-2, 1.0, 300000), (1e-2, 0.0, 0), (0.0, 0.0, 300000)])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_adam_clip_step_large_arena_with_tail(r, wd, max_norm, start):
    """n = 2 * 2048 * 1024 + r: the grid is capped at CTTS_ADAM_PARTIALS = 2048 workgroups, so the grid-stride loops of both kernels run
    twice, the second-stage reduction folds 2048 partials, and the n % 4 tail runs.  Six steps, then the same six again: same bits."""
    n = 2 * 2048 * 1024 + r
    a = adam_run(n, wd, max_norm, start, 6, seed=100 + r)
    b = adam_run(n, wd, max_norm, start, 6, seed=100 + r, check=False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("start", [0, 300000])
@pytest.mark.parametrize("max_norm", [1.0, 0.0])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("n", [3, 2051])
def test_adam_clip_step_small_arena_twenty_steps(n, wd, max_norm, start):
    a = adam_run(n, wd, max_norm, start, 20, seed=200 + n)
    b = adam_run(n, wd, max_norm, start, 20, seed=200 + n, check=False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_adam_clip_step_weight_decay_enters_after_the_clip():
    """g <- g * coef, THEN g <- g + weight_decay * p (include/ctts.h): with a clip coefficient of 1/50 and |p| ~ 1 the two orders differ
    by far more than the bar"""
    n = 2051
    g = torch.Generator().manual_seed(31)
    p0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g) * 50.0 / n ** 0.5
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p, m, v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    state, lr = torch.zeros(_lib.ADAM_STATE_FLOATS, device=DEV), torch.full((1,), 1e-2, device=DEV)
    K.adam_clip_step(p, grad.to(DEV), m, v, lr, B1, B2, EPS, 0.5, 1.0, state)
    L64.adam_clip_step(p64, grad.double(), m64, v64, 0, float(lr.item()), _f32(B1), _f32(B2), _f32(EPS), 0.5, 1.0)
    assert (m.cpu().double() - m64).abs().max().item() <= 1e-6 * m64.abs().max().item()
    assert (p.cpu().double() - p64).abs().max().item() <= ADAM_TOL * max(1.0, p64.abs().max().item())


def test_adam_clip_step_refuses_a_pointer_off_by_four_bytes():
    n = 64
    big = torch.zeros(n + 4, device=DEV)
    ok = [torch.zeros(n, device=DEV) for _ in range(3)]
    state, lr = torch.zeros(_lib.ADAM_STATE_FLOATS, device=DEV), torch.full((1,), 1e-3, device=DEV)
    for pos in range(4):
        args = list(ok)
        args.insert(pos, big[1:1 + n])
        assert args[pos].is_contiguous() and args[pos].data_ptr() % 16 == 4
        with pytest.raises(CttsError, match="16-byte aligned"):
            K.adam_clip_step(*args, lr, B1, B2, EPS, 0.0, 1.0, state)
    assert float(state.abs().max()) == 0.0 and float(big.abs().max()) == 0.0


def test_adam_clip_step_with_no_elements_leaves_everything_untouched():
    t = [torch.full((8,), 3.0, device=DEV) for _ in range(4)]
    state, lr = torch.full((_lib.ADAM_STATE_FLOATS,), 7.0, device=DEV), torch.full((1,), 1e-3, device=DEV)
    _lib.check(_lib.load().ctts_adam_clip_step(K._p(t[0]), K._p(t[1]), K._p(t[2]), K._p(t[3]), 0, K._p(lr), B1, B2, EPS, 0.0, 1.0,
                                               K._p(state), K._stream()), "ctts_adam_clip_step")
    torch.cuda.synchronize()
    assert float(state.min()) == 7.0 and float(state.max()) == 7.0 and all(float(x.min()) == 3.0 and float(x.max()) == 3.0 for x in t)


@pytest.mark.parametrize("n", [1031, 2 * 2048 * 1024 + 3])
def test_adam_clip_step_nan_norm_poisons_the_whole_step_like_clip_grad_norm(n):
    """include/ctts.h: with max_norm > 0 a NaN norm makes the clip coefficient NaN (torch's clamp keeps NaN; fminf would drop it), so
    every parameter and moment becomes NaN and state[2] reports NaN.  Without the clip only the element that holds the NaN is lost.
    Finite inputs with one NaN gradient; nothing here can fault."""
    g = torch.Generator().manual_seed(41)
    p0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01
    grad[n // 2] = float("nan")
    for max_norm in (1.0, 0.0):
        p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        p, m, v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        state, lr = torch.zeros(_lib.ADAM_STATE_FLOATS, device=DEV), torch.full((1,), 1e-3, device=DEV)
        K.adam_clip_step(p, grad.to(DEV), m, v, lr, B1, B2, EPS, 0.0, max_norm, state)
        total = L64.adam_clip_step(p64, grad.double(), m64, v64, 0, 1e-3, B1, B2, EPS, 0.0, max_norm)
        assert torch.isnan(total) and torch.isnan(state[2]).item() and float(state[1]) == 1.0
        for mine, ref in ((p, p64), (m, m64), (v, v64)):
            assert torch.equal(torch.isnan(mine).cpu(), torch.isnan(ref))
        assert int(torch.isnan(p64).sum()) == (n if max_norm > 0 else 1)


# ------------------------------------------------------------------------------------------------ graph replay
def test_one_linear_graph_replays_all_loss_kernels_and_adam_bit_exactly_on_changing_inputs():
    """variance_losses forward + backward, bin_loss, masked_loss, mel_l1_pair, forward_sum_nll (each with its backward) and one Adam step
    captured in this order into ONE graph on one stream (no parallel branches), warmed up on that stream first.  Replayed on three input
    sets copied into the static tensors, it returns the bits of the eager calls - the reason csrc/loss.hip exists is a torch reduction
    that did not."""
    B, Ts, Tm, NA = 4, 300, 600, 1_000_003
    src_lens, mel_lens = [300, 257, 40, 1], [600, 513, 77, 2]

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        b = var_batch(src_lens, mel_lens, Ts, Tm, seed)
        soft = torch.softmax(torch.randn(B, Tm, Ts, generator=g) * 3, dim=-1)
        hard = torch.zeros(B, Tm, Ts).scatter_(2, torch.randint(0, Ts, (B, Tm, 1), generator=g), 1.0) * (~b["mel_pad"])[:, :, None]
        n = 200_001
        mp, mt, mw = torch.randn(n, generator=g), torch.randn(n, generator=g), (torch.rand(n, generator=g) < 0.6).float()
        p1, p2, tgt = [torch.randn(B, Tm, 80, generator=g) for _ in range(3)]
        a = torch.randn(B, Tm, Ts, generator=g) * 2
        grad = torch.randn(NA, generator=g) * (seed % 3 + 0.5) / 1000.0
        d = dict(b, soft=soft, hard=hard, mp=mp, mt=mt, mw=mw, p1=p1, p2=p2, tgt=tgt, a=a, grad=grad,
                 w=torch.tensor(W_A if seed % 2 else W_B), lr=torch.tensor([1e-3 * (1 + seed % 4)]))
        return {k: v.to(DEV) for k, v in d.items()}

    lam_t = torch.tensor(LAMBDAS, dtype=torch.float32)
    il = torch.tensor(src_lens, dtype=torch.int32, device=DEV)
    ol = torch.tensor(mel_lens, dtype=torch.int32, device=DEV)
    one, two = torch.tensor(1.5, device=DEV), torch.tensor([0.7, -1.3], device=DEV)
    fsw = fs_weights(B).to(DEV)

    def step(d, opt):
        """the captured sequence; opt = (p, m, v, state) is updated in place"""
        ins = {k: d[k].detach().requires_grad_(True) for k in PRED + ("soft", "mp", "p1", "p2", "a")}
        out = []
        terms = ops.variance_losses(*[ins.get(k, d[k]) for k in ORDER], lam_t, 0, SIL_T)
        out += [terms] + list(torch.autograd.grad(terms, [ins[k] for k in PRED], grad_outputs=d["w"]))
        bl = ops.bin_loss(d["hard"], ins["soft"])
        out += [bl] + list(torch.autograd.grad(bl, [ins["soft"]], grad_outputs=one))
        ml = ops.masked_loss(ins["mp"], d["mt"], d["mw"], "l1")
        out += [ml] + list(torch.autograd.grad(ml, [ins["mp"]], grad_outputs=one))
        both = ops.mel_l1_pair(ins["p1"], ins["p2"], d["tgt"], d["mel_pad"])
        out += [both] + list(torch.autograd.grad(both, [ins["p1"], ins["p2"]], grad_outputs=two))
        nll = ops.forward_sum_nll(ins["a"], il, ol, -1.0)
        out += [nll] + list(torch.autograd.grad(nll, [ins["a"]], grad_outputs=fsw))
        K.adam_clip_step(opt[0], d["grad"], opt[1], opt[2], d["lr"], B1, B2, EPS, 1e-2, 1.0, opt[3])
        return out

    def new_opt():
        p = torch.randn(NA, generator=torch.Generator().manual_seed(77)).to(DEV)
        return [p, torch.zeros(NA, device=DEV), torch.zeros(NA, device=DEV), torch.zeros(_lib.ADAM_STATE_FLOATS, device=DEV)]

    static, opt_g, opt_e = make(50), new_opt(), new_opt()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on the capture stream: its workspace exists before the capture
        step(static, new_opt())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        outs = step(static, opt_g)
    torch.cuda.synchronize()
    for p, p0 in zip(opt_g, new_opt()):                          # the capture ran nothing
        assert torch.equal(p, p0)
    for seed in (51, 52, 53):
        fresh = make(seed)
        eager = [t.clone() for t in step(fresh, opt_e)]
        for k in static:
            static[k].copy_(fresh[k])
        graph.replay()
        torch.cuda.synchronize()
        assert len(outs) == len(eager) == 15
        for i, (x, y) in enumerate(zip(outs, eager)):
            assert torch.isfinite(y).all() and torch.equal(x, y), f"replay with input set {seed}: output {i} differs from the eager call"
        for i, (x, y) in enumerate(zip(opt_g, opt_e)):
            assert torch.equal(x[:3] if i == 3 else x, y[:3] if i == 3 else y), f"replay with input set {seed}: Adam tensor {i} differs"
    assert float(opt_g[3][1]) == 3.0
