"""Plain-torch restatement of everything downstream of the model outputs in a train step - the per-term oracle of
tests/test_loss_kernels_gpu.py (run in float64; the same code in float32 is the stock-torch yardstick the tests print).

Written from the formulas of include/ctts.h and the kernel headers of csrc/loss.hip, csrc/align.hip and csrc/optim.hip (which quote
model/loss.py of the reference): the eight variance / duration terms, BinLoss, the masked mean, the masked mel L1 pair, the aligner's
-temp * ||q - k||^2, the per-utterance CTC negative log-likelihood of ForwardSumLoss and the clip + Adam update.  Stock torch ops
with autograd on the CPU only; no product code and no oracle code is called.  tests/test_loss_restate_cpu.py pins it against
oracle.loss_restate.RefLoss and torch.optim.Adam."""
import torch
import torch.nn.functional as F

TERMS = ("pdur", "wdur", "sdur", "C", "uv", "f0_mean", "f0_std", "energy")
# The reference clamps a float32 tensor at 1e-12, so the bound it compares with is the float32 nearest to 1e-12 (as in the kernel).
BIN_CLAMP = float(torch.tensor(1e-12, dtype=torch.float32))


def word_ids(texts, sil_ids):
    """[B,Ts] int64: running count of silence tokens at every non-silence token, 0 at the silence tokens themselves.  Id 0 therefore
    collects the silences and the tokens in front of the first silence; it is dropped.  Pads (token 0) continue the last word."""
    sil = torch.zeros_like(texts, dtype=torch.bool)
    for s in sil_ids:
        sil = sil | (texts == int(s))
    sil = sil.long()
    return sil.cumsum(-1) * (1 - sil)


def variance_terms(log_d, cwt, f0_mean, f0_std, e_pred, dur, texts, src_pad, cwt_spec, uv, mel_pad, f0_mean_t, f0_std_t, e_tgt,
                   lambdas5, cwt_l2, sil_ids, dtype=torch.float64):
    """-> tensor [8] in the order of TERMS, each multiplied by its lambda (lambdas5 = ph, word, sent, f0, uv).  Arguments in the order
    of ops.variance_losses; the five predictions keep their autograd history (cast with .to(dtype) by the caller or here)."""
    lam_ph, lam_word, lam_sent, lam_f0, lam_uv = [float(x) for x in lambdas5]
    c = lambda t: t.to(dtype)                                                                          # noqa: E731
    log_d, cwt, f0_mean, f0_std, e_pred = c(log_d), c(cwt), c(f0_mean), c(f0_std), c(e_pred)
    cwt_spec, uv, f0_mean_t, f0_std_t, e_tgt = c(cwt_spec), c(uv), c(f0_mean_t), c(f0_std_t), c(e_tgt)
    B, Ts = log_d.shape
    nonpad = (~src_pad.bool()).to(dtype)
    mnonpad = (~mel_pad.bool()).to(dtype)
    dg = dur.to(dtype) * nonpad
    zero = torch.zeros((), dtype=dtype)
    pdur = ((log_d - torch.log(dg + 1)) ** 2 * nonpad).sum() / nonpad.sum() * lam_ph
    lin = (torch.exp(log_d) - 1).clamp(min=0)                               # linear predicted durations, pads included
    wdur = zero
    if lam_word > 0:
        wid = word_ids(texts, sil_ids)
        wp = torch.zeros(B, Ts + 1, dtype=dtype).scatter_add(1, wid, lin)[:, 1:]
        wg = torch.zeros(B, Ts + 1, dtype=dtype).scatter_add(1, wid, dg)[:, 1:]
        wn = (wg > 0).to(dtype)
        wdur = ((torch.log(wp + 1) - torch.log(wg + 1)) ** 2 * wn).sum() / wn.sum() * lam_word
    sdur = zero
    if lam_sent > 0:
        sdur = ((torch.log(lin.sum(-1) + 1) - torch.log(dg.sum(-1) + 1)) ** 2).mean() * lam_sent
    df = cwt[:, :, :10] - cwt_spec
    cterm = ((df ** 2) if cwt_l2 else df.abs()).mean() * lam_f0             # padded frames included by design
    bce = F.binary_cross_entropy_with_logits(cwt[:, :, 10], uv, reduction="none")          # slope sigmoid(x) - y, also at x == 0
    uvterm = (bce * mnonpad).sum() / mnonpad.sum() * lam_uv
    f0m = (f0_mean - f0_mean_t).abs().mean() * lam_f0
    f0s = (f0_std - f0_std_t).abs().mean() * lam_f0
    energy = ((e_pred - e_tgt).abs() * nonpad).sum() / nonpad.sum()
    return torch.stack([pdur, wdur, sdur, cterm, uvterm, f0m, f0s, energy])


def bin_loss(hard, soft, dtype=torch.float64):
    """-sum(log(clamp(soft, 1e-12)) * hard) / sum(hard)"""
    hard, soft = hard.to(dtype), soft.to(dtype)
    return -(torch.log(soft.clamp(min=BIN_CLAMP)) * hard).sum() / hard.sum()


def masked_mean(pred, target, weight, kind, dtype=torch.float64):
    """sum_i w_i l(p_i, t_i) / sum_i w_i with l = |p - t| ("l1"), (p - t)^2 ("l2") or BCE with logits ("bce")"""
    p, t, w = pred.to(dtype), target.to(dtype), weight.to(dtype)
    if kind == "l1":
        l = (p - t).abs()
    elif kind == "l2":
        l = (p - t) ** 2
    else:
        l = F.binary_cross_entropy_with_logits(p, t, reduction="none")
    return (l * w).sum() / w.sum()


def mel_l1_pair(p1, p2, target, pad, dtype=torch.float64):
    """rows with pad != 0 count as zeros, w[row] = (sum_c |target[row, c]| != 0); -> ([2] losses sums[k] / (C * sums[2]), sums [3], w)"""
    keep = (~pad.bool()).unsqueeze(-1).to(dtype)
    t = target.to(dtype) * keep
    w = (t.abs().sum(-1, keepdim=True) != 0).to(dtype)
    s1 = ((p1.to(dtype) * keep - t).abs() * w).sum()
    s2 = ((p2.to(dtype) * keep - t).abs() * w).sum()
    sw = w.sum()
    Cc = target.shape[-1]
    return torch.stack([s1, s2]) / (Cc * sw), torch.stack([s1.detach(), s2.detach(), sw]), w[..., 0]


def neg_sqdist(q, k, temp, dtype=torch.float64):
    """q [B,Tq,C], k [B,Tk,C] -> [B,Tq,Tk] = -temp * sum_c (q[b,t,c] - k[b,s,c])^2"""
    q, k = q.to(dtype), k.to(dtype)
    return -temp * ((q[:, :, None, :] - k[:, None, :, :]) ** 2).sum(-1)


def forward_sum_nll(attn_logprob, in_lens, out_lens, blank_logprob=-1.0, dtype=torch.float64):
    """attn_logprob [B,Tm,Ts] -> (nll [B] with +inf where the K_b tokens do not fit into the T_b frames, nll0 [B] = the same with the
    infinities zeroed and carrying the autograd history).  Per utterance: CTC negative log-likelihood of the targets 1..K_b under
    log_softmax([blank, a[t, :K_b]]) over the first T_b frames."""
    a = F.pad(attn_logprob.to(dtype), (1, 0), value=float(blank_logprob))
    nll, nll0 = [], []
    for b in range(a.shape[0]):
        K_, T_ = int(in_lens[b]), int(out_lens[b])
        lp = torch.log_softmax(a[b, :T_, :K_ + 1], dim=-1).unsqueeze(1)                     # [T, 1, K+1]
        args = (lp, torch.arange(1, K_ + 1)[None], torch.tensor([T_]), torch.tensor([K_]))
        nll0.append(F.ctc_loss(*args, blank=0, reduction="sum", zero_infinity=True))
        with torch.no_grad():
            nll.append(F.ctc_loss(*args, blank=0, reduction="sum", zero_infinity=False))
    return torch.stack(nll), torch.stack(nll0)


def adam_clip_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, max_norm):
    """One update of include/ctts.h's ctts_adam_clip_step on flat tensors, in place on p, m, v (any dtype; float64 is the oracle):
         total = ||g||_2 ; g <- g * min(1, max_norm / (total + 1e-6))      (max_norm <= 0: no clipping)
         g <- g + weight_decay * p ; m <- b1 m + (1 - b1) g ; v <- b2 v + (1 - b2) g^2
         p <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)     with t = step + 1
    A NaN norm makes the clip coefficient NaN (min(1, NaN) = NaN, as torch.clamp): the whole step is poisoned.  -> total norm."""
    total = g.pow(2).sum().sqrt()
    gg = g
    if max_norm > 0:
        gg = g * torch.clamp(max_norm / (total + 1e-6), max=1.0)
    gg = gg + weight_decay * p
    m.mul_(beta1).add_(gg, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gg, gg, value=1 - beta2)
    t = step + 1
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    p.sub_(lr / bc1 * (m / (v.sqrt() / bc2 ** 0.5 + eps)))
    return total
