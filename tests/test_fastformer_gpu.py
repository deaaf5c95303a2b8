"""GPU: block_type "fastformer" - the additive-attention kernels (csrc/fastformer.hip) against float64, the G18 reference fixtures, the
full-size decoder stack against tests/fastformer_restate.py, tied-weight gradients and bit-reproducible graph replay."""
import os

import numpy as np
import pytest
import torch

import ctts_amd
from ctts_amd import kernels as K
from ctts_amd.configs import get_configs
from ctts_amd.synthetic import make_batch, to_device, as_model_args
from oracle.weights import _hash_uniform
from tests import fastformer_restate as FR
from tests.test_fastformer_cpu import tied_from_layer0
from tests.util import load_golden, closed_form_sd, batch_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEL_TOL = 1e-3
DIV = float(2 ** 0.5)


def _build(sd=None, train=False):
    pre, mc, tc = get_configs()
    mc["block_type"] = "fastformer"
    m = ctts_amd.CompTransTTS(pre, mc, tc)
    if sd is not None:
        m.load_state_dict(sd)
    m = m.to(DEV)
    m.train(train)
    return m, (pre, mc, tc)


def _no_dropout(m):
    for sub in m.modules():
        if hasattr(sub, "dropout"):
            sub.dropout = 0.0


def _maxerr(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max())


def _args(g):
    b = to_device(batch_from_golden(g), DEV)
    return (b["speakers"], b["texts"], b["src_lens"], b["max_src_len"], b["mels"], b["mel_lens"], b["max_mel_len"], b["p_targets"],
            b["e_targets"], b["d_targets"], None, b["spker_embeds"])


# ---------------------------------------------------------------------------------------------------------------- kernels vs fp64
def _pool_case(B, T, lens, seed, H=128, C=256):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, T, H, generator=g, dtype=torch.float64) * 3
    V = torch.randn(B, T, C, generator=g, dtype=torch.float64)
    return s, V, torch.tensor(lens, dtype=torch.int32)


@pytest.mark.parametrize("T", [1, 2, 63, 1000, 1024])
@pytest.mark.parametrize("padded", [False, True])
def test_pool_forward_and_backward_vs_fp64(T, padded):
    B, H, C = 3, 128, 256
    lens = [T, max(1, T // 2), max(1, T - 1)] if padded else [T] * B
    s, V, ln = _pool_case(B, T, lens, seed=T + 7 * padded)
    s.requires_grad_(True)
    V.requires_grad_(True)
    p_ref = FR.pool(s, V, ln, C // H)
    dp = torch.randn(B, C, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    p_ref.backward(dp)
    sd, Vd, lnd = s.detach().float().to(DEV).view(B * T, H), V.detach().float().to(DEV).view(B * T, C), ln.to(DEV)
    p, st = K.fastformer_pool_fwd(sd, Vd, lnd, B, T, H, DIV)
    dV, ds = K.fastformer_pool_bwd(dp.float().to(DEV), p, st, sd, Vd, lnd, B, T, H, DIV)
    assert _maxerr(p, p_ref) <= 1e-5 * max(1.0, float(p_ref.abs().max()))
    assert _maxerr(dV.view(B, T, C), V.grad) <= 1e-5 * max(1.0, float(V.grad.abs().max()))
    assert _maxerr(ds.view(B, T, H), s.grad) <= 1e-5 * max(1.0, float(s.grad.abs().max()))


def test_pool_on_a_column_slice_and_in_place_accumulation():
    """s may be a column slice of a wider matrix (row stride > H); dV_in is added in place"""
    B, T, H, C = 3, 70, 128, 256
    s, V, ln = _pool_case(B, T, [70, 40, 9], seed=3)
    wide = torch.zeros(B * T, 2 * H, device=DEV)
    wide[:, H:] = s.float().to(DEV).view(B * T, H)
    p1, st1 = K.fastformer_pool_fwd(wide[:, H:], V.float().to(DEV).view(B * T, C), ln.to(DEV), B, T, H, DIV)
    p2, st2 = K.fastformer_pool_fwd(s.float().to(DEV).view(B * T, H), V.float().to(DEV).view(B * T, C), ln.to(DEV), B, T, H, DIV)
    assert torch.equal(p1, p2) and torch.equal(st1, st2)
    dp = torch.randn(B, C, device=DEV)
    base = torch.randn(B * T, C, device=DEV)
    acc = base.clone()
    dV, _ = K.fastformer_pool_bwd(dp, p2, st2, wide[:, H:], V.float().to(DEV).view(B * T, C), ln.to(DEV), B, T, H, DIV, dV_in=acc)
    ref, _ = K.fastformer_pool_bwd(dp, p2, st2, wide[:, H:], V.float().to(DEV).view(B * T, C), ln.to(DEV), B, T, H, DIV)
    assert dV.data_ptr() == acc.data_ptr() and _maxerr(dV, base + ref) <= 1e-6 * float((base + ref).abs().max())      # one fused multiply-add


def test_padding_only_pooling_is_exact_on_integers():
    """an utterance with padding pools over its PADDED rows only (valid frames get -10000 and weight exactly 0): with equal logits on
    the 8 padded rows and integer values the result is their exact mean"""
    B, T, H, C = 3, 24, 128, 256
    lens = torch.tensor([16, 16, 16], dtype=torch.int32)
    g = torch.Generator().manual_seed(1)
    s = torch.zeros(B, T, H)
    s[:, :16] = torch.randint(-50, 50, (B, 16, H), generator=g).float()     # valid frames: anything, they must not count
    V = torch.randint(-64, 64, (B, T, C), generator=g).float()
    p, _ = K.fastformer_pool_fwd(s.to(DEV).view(B * T, H), V.to(DEV).view(B * T, C), lens.to(DEV), B, T, H, DIV)
    assert torch.equal(p.cpu(), V[:, 16:].sum(1) / 8)


def test_minus_10000_rounds_unpadded_logits():
    """no padding: every logit gets -10000 in fp32, which rounds s / sqrt(2) in [0, 3e-4) to exactly -10000 - the weights become
    uniform (64 rows, integer values: exact mean), unlike a softmax of the unrounded logits"""
    B, T, H, C = 1, 64, 128, 256
    g = torch.Generator().manual_seed(2)
    s = torch.rand(B, T, H, generator=g) * 3e-4
    V = torch.randint(-1000, 1000, (B, T, C), generator=g).float()
    p, _ = K.fastformer_pool_fwd(s.to(DEV).view(B * T, H), V.to(DEV).view(B * T, C), torch.tensor([T], dtype=torch.int32, device=DEV),
                                 B, T, H, DIV)
    assert torch.equal(p.cpu(), V.sum(1) / 64)
    unrounded = (torch.softmax(s.double() / DIV, 1).repeat_interleave(2, 2) * V.double()).sum(1)
    assert float((unrounded - p.cpu().double()).abs().max()) > 1e-4


def test_result_changes_when_only_padded_rows_change():
    """the padded rows are part of the semantics: changing them alone moves the valid outputs of the block"""
    m, _ = _build(tied_from_layer0(closed_form_sd("LJSpeech", "fastformer")))
    dec = m.decoder
    x = torch.randn(2, 40, 256, device=DEV)
    mask = torch.arange(40, device=DEV)[None, :] >= torch.tensor([40, 25], device=DEV)[:, None]
    with torch.no_grad():
        y1, _ = dec(x, mask)
        x2 = x.clone()
        x2[1, 25:] += 3.0
        y2, _ = dec(x2, mask.clone())
        y1b, _ = dec(x.clone(), mask.clone())
    assert torch.equal(y1, y1b)                    # deterministic: any difference below comes from the padded rows alone
    assert torch.equal(y1[0], y2[0])
    assert float((y1[1, :25] - y2[1, :25]).abs().max()) > 0.0
    assert float(y2[1, 25:].abs().max()) == 0.0


def test_broadcast_products_and_column_reductions_vs_fp64():
    B, T, C = 5, 1000, 256
    g = torch.Generator().manual_seed(4)
    X, p, dY1, dY2, dXin = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((B * T, C), (B, C), (B * T, C), (B * T, C), (B * T, C)))
    Y = K.fastformer_bcast(X.float().to(DEV), p.float().to(DEV), B, T)
    assert _maxerr(Y, (X.view(B, T, C) * p[:, None]).view(B * T, C)) <= 1e-6 * float(Y.abs().max())
    dX, dp = K.fastformer_bcast_bwd(dY1.float().to(DEV), X.float().to(DEV), p.float().to(DEV), B, T, dY2=dY2.float().to(DEV),
                                    dX_in=dXin.float().to(DEV))
    dy = (dY1 + dY2).view(B, T, C)
    assert _maxerr(dX, dXin + (dy * p[:, None]).view(B * T, C)) <= 1e-5 * 10
    assert _maxerr(dp, (dy * X.view(B, T, C)).sum(1)) <= 1e-5 * float((dy * X.view(B, T, C)).sum(1).abs().max()) + 1e-4


def test_residual_dropout_forward_backward_agree():
    x, t = torch.randn(300, 256, device=DEV), torch.randn(300, 256, device=DEV)
    rs = (torch.arange(300, device=DEV) % 7 != 0).float()
    seed = torch.tensor([1234567], dtype=torch.int64, device=DEV)
    y = K.fastformer_resdrop(x, t, rs, 0.2, seed, 3)
    keep = (y - rs[:, None] * x) != 0
    frac = float(keep[rs > 0].float().mean())
    assert 0.75 < frac < 0.85
    dx, dt = K.fastformer_resdrop_bwd(torch.ones_like(t), rs, 0.2, seed, 3)
    assert torch.equal(dx, rs[:, None].expand_as(dx))
    assert torch.allclose(dt, torch.where(keep, rs[:, None] / 0.8, torch.zeros_like(dt)))


# ------------------------------------------------------------------------------------------------------------- G18 fixtures
def _check_outputs(out, g):
    mel, post, p_pred, e_pred, log_d, d_rounded, src_mask, mel_mask, src_lens, mel_lens = out[:10]
    errs = {"mel": _maxerr(mel, g["out.mel"]), "postnet_mel": _maxerr(post, g["out.postnet_mel"]), "log_d": _maxerr(log_d, g["out.log_d"]),
            "e_pred": _maxerr(e_pred, g["out.e_pred"]), "cwt": _maxerr(p_pred["cwt"], g["out.cwt"]),
            "f0_mean": _maxerr(p_pred["f0_mean"], g["out.f0_mean"]), "f0_std": _maxerr(p_pred["f0_std"], g["out.f0_std"])}
    print("fastformer max-abs vs reference golden:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= MEL_TOL, (k, v)
    assert np.array_equal(d_rounded.cpu().numpy(), g["out.d_rounded"])
    assert np.array_equal(mel_mask.cpu().numpy(), g["out.mel_mask"])


@pytest.mark.parametrize("name,kw", [("g18_fastformer_eval", {}), ("g18_fastformer_infer", dict(p_control=1.1, e_control=0.9, d_control=2.0))])
def test_g18_fastformer_eval_and_infer_match_reference(name, kw):
    g = load_golden(name)
    m, _ = _build(tied_from_layer0(closed_form_sd("LJSpeech", "fastformer")))
    with torch.no_grad():
        out = m(*_args(g), **kw)
    _check_outputs(out, g)
    assert _maxerr(out[0], g["out.mel"]) <= MEL_TOL


def test_g18_fastformer_train_gradients_match_reference():
    g = load_golden("g18_fastformer_train_nodrop")
    m, _ = _build(tied_from_layer0(closed_form_sd("LJSpeech", "fastformer")), train=True)
    _no_dropout(m)
    out = m(*_args(g))
    _check_outputs(out, g)

    def pseudo(name, shape):
        return torch.from_numpy(_hash_uniform("probe." + name, int(np.prod(shape))).reshape(shape)).float().to(DEV)
    mel, post, p_pred, e_pred, log_d = out[:5]
    loss = ((post * pseudo("post", post.shape)).sum() + (mel * pseudo("mel", mel.shape)).sum()
            + (log_d * pseudo("logd", log_d.shape)).sum() + (e_pred * pseudo("e", e_pred.shape)).sum()
            + (p_pred["cwt"] * pseudo("cwt", p_pred["cwt"].shape)).sum()
            + (p_pred["f0_mean"] * 0.7).sum() + (p_pred["f0_std"] * -0.3).sum())
    loss.backward()
    worst, n = ("", 0.0), 0
    for k, p in m.named_parameters():
        if "grad.stat." + k not in g:
            continue
        gs = g["grad.stat." + k]
        gr = p.grad.flatten() if p.grad is not None else torch.zeros(p.numel(), device=DEV)
        scale = max(1.0, float(gs[1]))
        e = max(_maxerr(gr[:64], g["grad.head." + k]) / scale, abs(float(gr.double().pow(2).sum().sqrt()) - gs[1]) / scale)
        if e > worst[1]:
            worst = (k, e)
        n += 1
    print("fastformer worst relative gradient error:", worst, "over", n, "parameters")
    assert n >= 200 and worst[1] < 2e-3, worst


# ---------------------------------------------------------------------------------------------------------------- full size
def _decoder_case(B, lens, T, seed):
    torch.manual_seed(seed)
    m, (pre, mc, tc) = _build(train=True)
    _no_dropout(m)
    dec = m.decoder
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 256, generator=g)
    pad = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
    dy = torch.randn(B, min(T, 1000), 256, generator=g)
    return m, dec, x, pad, dy


def test_full_size_decoder_forward_and_gradients_vs_restate():
    """B = 16 canonical utterances, frames capped at 1000 (the training crop): forward and every gradient of the 6-layer decoder stack
    within 2e-3 of each tensor's max against the float64 restatement"""
    from ctts_amd.synthetic import CANONICAL_SRC_LENS
    lens = [min(1000, 8 * l) for l in CANONICAL_SRC_LENS]
    T = max(lens)
    m, dec, x, pad, dy = _decoder_case(16, lens, T, seed=11)
    xd = x.to(DEV).requires_grad_(True)
    y, _ = dec(xd, pad.to(DEV))
    y.backward(dy.to(DEV))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = {k: v for k, v in m.state_dict(keep_vars=True).items() if k.startswith("decoder.")}
    layers = FR.stack_params({k: v.detach() for k, v in sd.items()}, "decoder", 6)
    leaves = [t for A, Fp in layers for d in (A, Fp) for pair in d.values() for t in pair]
    for t in leaves:
        t.requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    pos = dec.position_enc[0, :T].detach().cpu().double()
    y64 = FR.stack_forward(x64 + pos, pad, layers, 128)
    y64.backward(dy.double())
    assert _maxerr(y, y64) <= 2e-3 * float(y64.abs().max())
    assert _maxerr(xd.grad, x64.grad) <= 2e-3 * float(x64.grad.abs().max())
    names = ["norm", "query", "key", "to_q_attn_logits", "to_k_attn_logits", "transform"]
    for i, (A, Fp) in enumerate(layers):
        sub = dec.layer_stack.layers[i]
        for n in names + ["ffn"]:
            if n == "ffn":
                pairs = [(sub[1].fn.w_1, Fp["w_1"]), (sub[1].fn.w_2, Fp["w_2"]), (sub[1].norm, Fp["norm"])]
            elif n == "norm":
                pairs = [(sub[0].norm, A["norm"])]
            elif n.startswith("to_"):
                continue                                   # tied: compared as sums below
            else:
                pairs = [(getattr(sub[0].fn, n), A[n])]
            for mod, (w, b) in pairs:
                for got, ref in ((mod.weight.grad, w.grad), (mod.bias.grad, b.grad)):
                    assert _maxerr(got.reshape(ref.shape), ref) <= 2e-3 * float(ref.abs().max()), (i, n)
    # a tied weight's gradient is the sum of its per-layer contributions.  The logit biases shift every logit of a head alike, which the
    # softmax ignores: their exact gradient is zero, so their bar is set by the weight gradient of the same projection
    for n in ("to_q_attn_logits", "to_k_attn_logits"):
        mod = getattr(dec.layer_stack.layers[0][0].fn, n)
        wref = sum(A[n][0].grad for A, _ in layers)
        for got, k in ((mod.weight.grad, 0), (mod.bias.grad, 1)):
            ref = sum(A[n][k].grad for A, _ in layers)
            assert _maxerr(got, ref) <= 2e-3 * max(float(ref.abs().max()), float(wref.abs().max())), n


def test_tied_weight_gradient_is_the_sum_over_layers():
    """the tied logit projections collect every layer's contribution: the gradient equals the sum of the per-layer gradients of an
    untied copy (each layer's own leaf), under plain autograd and under gradient-accumulation fusion into the flat arena"""
    from ctts_amd import ops
    from ctts_amd.dp import FlatGradArena
    m, dec, x, pad, dy = _decoder_case(3, [50, 37, 20], 50, seed=12)
    mask = pad.to(DEV)
    y, _ = dec(x.to(DEV), mask)
    y.backward(dy.to(DEV))
    tied = dec.layer_stack.layers[0][0].fn.to_k_attn_logits
    g_plain = tied.weight.grad.clone()
    # per-layer contributions: give every layer its own copy of the projection
    shared = [(l[0].fn.to_q_attn_logits, l[0].fn.to_k_attn_logits) for l in dec.layer_stack.layers]
    import copy
    copies = [copy.deepcopy(tied) for _ in dec.layer_stack.layers]
    for l, c in zip(dec.layer_stack.layers, copies):
        l[0].fn.to_k_attn_logits = c
    try:
        y2, _ = dec(x.to(DEV), mask.clone())
        y2.backward(dy.to(DEV))
        total = sum(c.weight.grad.double() for c in copies)
    finally:
        for l, (q, k) in zip(dec.layer_stack.layers, shared):
            l[0].fn.to_k_attn_logits = k
    assert _maxerr(g_plain, total) <= 1e-5 * float(total.abs().max())
    assert torch.equal(y, y2)
    # fused accumulation straight into a flat gradient arena (the train step's path), with and without the weight-gradient side stream
    for side in (False, True):
        arena = FlatGradArena(dec.parameters())
        ops.set_grad_accumulation_fusion(True)
        ops.set_wgrad_stream(torch.cuda.Stream() if side else None)
        try:
            y3, _ = dec(x.to(DEV), mask.clone())
            y3.backward(dy.to(DEV))
        finally:
            ops.set_grad_accumulation_fusion(False)
            ops.set_wgrad_stream(None)
        torch.cuda.synchronize()
        assert _maxerr(tied.weight.grad, g_plain) <= 1e-5 * float(g_plain.abs().max()), side
        assert arena.flat.abs().sum() > 0


def test_captured_train_step_replays_bit_identically():
    from ctts_amd.loss import CompTransTTSLoss, ScheduledOptim
    from ctts_amd.trainer import TrainStep

    def run():
        torch.manual_seed(1234)
        m, (pre, mc, tc) = _build(train=True)
        loss_fn, optim = CompTransTTSLoss(pre, mc, tc).to(DEV), ScheduledOptim(m, tc, mc, 50000, capturable=True)
        batch = to_device(make_batch([60, 41, 33, 17], 8, seed=3), DEV)
        step = TrainStep(m, loss_fn, optim, as_model_args(batch), world=1, use_graph=True)
        step.capture(warmup=2)
        losses = []
        for i in range(2):
            step()
            losses.append(float(step.loss_val))
        torch.cuda.synchronize()
        return losses, step.flat_grad.clone(), step.fadam.flat_param.clone()
    a, b = run(), run()
    assert all(np.isfinite(a[0]))
    assert a[0] == b[0]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
