"""Plain-torch float64 restatement of the Fastformer block (reference model/transformers/fastformer.py FastAttention / FFTBlock), the
per-shape oracle for sizes too large for fixtures.  Differentiable (autograd in float64).

The one fp32 effect of the reference that is part of its result is kept: the logits are `score / sqrt(D) + mask` evaluated in fp32,
where mask = -10000 on valid frames and 0 on padding - the add rounds valid-frame logits to the 2^-10 grid.  The rounding enters as a
constant correction, so gradients flow as through the exact expression."""
import torch
import torch.nn.functional as F


def logits(s, lens, D):
    """s [B, T, H] float64 -> z [B, T, H]: fp32-rounded s / sqrt(D) + (t < lens[b] ? -10000 : 0), gradient of the exact expression"""
    B, T, _ = s.shape
    m = torch.where(torch.arange(T)[None, :] < lens.view(-1, 1).cpu(), -10000.0, 0.0).to(torch.float64)[:, :, None]
    div = float(D) ** 0.5
    z = s / div + m
    z32 = (s.detach().float() / torch.tensor(div, dtype=torch.float32)) + m.float()
    return z + (z32.double() - z.detach())


def pool(s, V, lens, D):
    """alpha = softmax_t(logits) per head, p[b, c] = sum_t alpha[b, t, c // D] V[b, t, c] -> p [B, C]"""
    alpha = torch.softmax(logits(s, lens, D), dim=1)               # [B, T, H]
    return (alpha.repeat_interleave(D, dim=2) * V).sum(1)


def fast_attention(h, lens, P, H):
    """h [B, T, C] -> transform(pk * Q) + Q (FastAttention.forward without its dropout); P: dict with query / key / to_q_attn_logits /
    to_k_attn_logits / transform -> (weight, bias)"""
    C = h.shape[-1]
    D = C // H
    Q = F.linear(h, *P["query"])
    Kt = F.linear(h, *P["key"])
    pq = pool(F.linear(Q, *P["to_q_attn_logits"]), Q, lens, D)
    QK = Kt * pq[:, None, :]
    pk = pool(F.linear(QK, *P["to_k_attn_logits"]), QK, lens, D)
    return F.linear(pk[:, None, :] * Q, *P["transform"]) + Q


def layer(x, lens, pad, A, Fp, H):
    """one FFTBlock layer (fastformer.py:160-167): x + PreNorm(FastAttention), masked_fill; x + PreNorm(FFN), masked_fill"""
    C = x.shape[-1]
    keep = (~pad).to(x.dtype)[:, :, None]
    x = (x + fast_attention(F.layer_norm(x, (C,), *A["norm"], 1e-5), lens, A, H)) * keep
    h = F.layer_norm(x, (C,), *Fp["norm"], 1e-5).transpose(1, 2)
    w1, b1 = Fp["w_1"]
    w2, b2 = Fp["w_2"]
    g = F.conv1d(F.gelu(F.conv1d(h, w1, b1, padding=(w1.shape[2] - 1) // 2)), w2, b2)
    return (x + g.transpose(1, 2)) * keep


def stack_params(sd, prefix, n_layers, dtype=torch.float64):
    """per-layer parameter dicts of a `<prefix>.layer_stack` from a state dict (tied keys read per layer)"""
    def t(k):
        return sd[k].detach().to(dtype).cpu()
    out = []
    for i in range(n_layers):
        a, f = f"{prefix}.layer_stack.layers.{i}.0.", f"{prefix}.layer_stack.layers.{i}.1."
        A = {"norm": (t(a + "norm.weight"), t(a + "norm.bias"))}
        for n in ("query", "key", "to_q_attn_logits", "to_k_attn_logits", "transform"):
            A[n] = (t(a + f"fn.{n}.weight"), t(a + f"fn.{n}.bias"))
        Fp = {"norm": (t(f + "norm.weight"), t(f + "norm.bias")), "w_1": (t(f + "fn.w_1.weight"), t(f + "fn.w_1.bias")),
              "w_2": (t(f + "fn.w_2.weight"), t(f + "fn.w_2.bias"))}
        out.append((A, Fp))
    return out


def stack_forward(x, pad, layers, H):
    """x [B, T, C] float64 (embedding + position table already added), pad [B, T] bool (True = padding)"""
    lens = (~pad).sum(1)
    for A, Fp in layers:
        x = layer(x, lens, pad, A, Fp, H)
    return x
