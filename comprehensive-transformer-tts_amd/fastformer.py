"""`fastformer` block plugin (reference: model/transformers/fastformer.py, wuch15's FastAttention) on the gfx950 kernels.

Plugin contract (CompTransTTS.py:19-39): `TextEncoder(config).forward(tokens, pad_mask) -> (enc, word_emb)`,
`Decoder(config).forward(x, pad_mask) -> (dec, mask)`, both expose `.d_model`; state-dict keys follow the reference
(`layer_stack.layers.{i}.0.{norm,fn}...` for the attention, `layer_stack.layers.{i}.1.{norm,fn}...` for the FFN).

Behaviour kept bug-compatible with the reference:
  * `FastAttention(d_model, d_head, n_head)` swaps its arguments: the shipped config runs d_head = 128 heads of size d_model / d_head = 2,
    the logit projections are Linear(256 -> 128) and the scores are divided by sqrt(2);
  * the pooling mask is inverted: -10000 is added on VALID frames and 0 on padding, over the full padded length (csrc/fastformer.hip);
  * `to_q_attn_logits` / `to_k_attn_logits` are ONE module per stack, tied across its layers (listed under every layer's key);
  * each sub-layer is x = x + PreNorm(fn)(x), then masked_fill(pad, 0); the attention's own output is dropout(transform(WV) + Q);
  * the decoder crops to max_seq_len in training; eval beyond max_seq_len builds a fresh sinusoid table.
"""
import math

import torch
import torch.nn as nn

from . import ops
from .configs import N_SYMBOLS
from .conformer import interleaved_sinusoid_table
from .model import _Linear, _Norm, _Conv, mask_aux


class _FastAttentionParams(nn.Module):
    """fastformer.py FastAttention: registration order query, to_q_attn_logits, key, to_k_attn_logits, transform"""

    def __init__(self, dim, n_heads, q_logits=None, k_logits=None):
        super().__init__()
        self.num_attention_heads = n_heads
        self.query = _Linear(dim, dim)
        self.to_q_attn_logits = q_logits if q_logits is not None else _Linear(dim, n_heads)
        self.key = _Linear(dim, dim)
        self.to_k_attn_logits = k_logits if k_logits is not None else _Linear(dim, n_heads)
        self.transform = _Linear(dim, dim)


class _FFNParams(nn.Module):
    """fastformer.py PositionwiseFeedForward: w_1 Conv1d(d, d_inner, k0, pad (k0-1)/2), w_2 Conv1d(d_inner, d, k1)"""

    def __init__(self, d_in, d_hid, ksize):
        super().__init__()
        assert ksize[1] == 1, "fastformer FFN: only a pointwise second convolution is supported"
        self.w_1 = _Conv(d_in, d_hid, ksize[0])
        self.w_2 = _Conv(d_hid, d_in, ksize[1])


class _PreNorm(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = _Norm(dim)
        self.fn = fn


class FFTBlock(nn.Module):
    """fastformer.py FFTBlock: `layers[i] = [PreNorm(LN, FastAttention), PreNorm(LN, FFN)]`, logit projections tied to layer 0's"""

    def __init__(self, depth, d_model, n_heads, d_inner, ksize, dropout):
        super().__init__()
        self.n_heads, self.dropout, self.ksize = n_heads, dropout, ksize
        self.layers = nn.ModuleList()
        q_lg = k_lg = None
        for _ in range(depth):
            attn = _FastAttentionParams(d_model, n_heads, q_lg, k_lg)
            q_lg, k_lg = attn.to_q_attn_logits, attn.to_k_attn_logits
            self.layers.append(nn.ModuleList([_PreNorm(d_model, attn), _PreNorm(d_model, _FFNParams(d_model, d_inner, ksize))]))
        self.drop_ctx = None
        self._cut_prefix = None

    def forward(self, x, mask):
        nonpad, lens = mask_aux(mask)
        B, T, C = x.shape
        p = self.dropout if self.training else 0.0
        drop = self.drop_ctx if p > 0 else None
        for li, (attn, ff) in enumerate(self.layers):
            if self._cut_prefix is not None:
                x = ops.stage_cut(x, f"{self._cut_prefix}.{li}")
            a = attn.fn
            h, xr = ops.layer_norm_res(x, attn.norm.weight, attn.norm.bias, 1e-5)
            t = ops.fast_attention(h, lens, a.num_attention_heads, a.query.weight, a.query.bias, a.key.weight, a.key.bias,
                                   a.to_q_attn_logits.weight, a.to_q_attn_logits.bias, a.to_k_attn_logits.weight, a.to_k_attn_logits.bias,
                                   a.transform.weight, a.transform.bias)
            x = ops.residual_dropout(xr, t, nonpad, p, drop)
            f = ff.fn
            h, xr = ops.layer_norm_res(x, ff.norm.weight, ff.norm.bias, 1e-5, planes_for=(f.w_1.weight.shape[0], f.w_1.weight.shape[2]))
            link = ops.EpiLink()        # GELU' rides in w_2's data-gradient GEMM
            g = ops.conv1d(h, f.w_1.weight, f.w_1.bias, act=ops.ACT_GELU, link=link, link_role=1)
            x = ops.linear(g, f.w_2.weight.view(C, -1), f.w_2.bias, residual=xr, rowscale=nonpad, p_drop=p, drop=drop, link=link,
                           link_role=2)
        return x


class _FastformerStack(nn.Module):
    def __init__(self, config, which):
        super().__init__()
        c = config["transformer"]
        self.d_model = c[f"{which}_hidden"]
        self.max_seq_len = config["max_seq_len"]
        d_head = c[f"{which}_hidden"] // c[f"{which}_head"]          # passed as FastAttention's head COUNT (fastformer.py:27-31,171)
        if which == "encoder":
            self.src_word_emb = nn.Embedding(N_SYMBOLS + 1, self.d_model, padding_idx=0)
        self.position_enc = nn.Parameter(interleaved_sinusoid_table(self.max_seq_len + 1, self.d_model).unsqueeze(0), requires_grad=False)
        self.layer_stack = FFTBlock(c[f"{which}_layer"], self.d_model, d_head, c["conv_filter_size"], c["conv_kernel_size"],
                                    c[f"{which}_dropout"])

    @property
    def drop_ctx(self):
        return self.layer_stack.drop_ctx

    @drop_ctx.setter
    def drop_ctx(self, v):
        self.layer_stack.drop_ctx = v

    def _pos(self, T, device):
        if not self.training and T > self.max_seq_len:
            return interleaved_sinusoid_table(T, self.d_model).to(device)
        return self.position_enc[0, :T]

    def run(self, x, mask):
        self.layer_stack._cut_prefix = getattr(self, "_cut_prefix", None)
        return self.layer_stack(x, mask)


class TextEncoder(_FastformerStack):
    """fastformer.py:16-68"""

    def __init__(self, config):
        super().__init__(config, "encoder")

    def forward(self, src_seq, mask):
        emb = ops.embedding(src_seq, self.src_word_emb.weight, 0)
        pos = self._pos(src_seq.shape[1], emb.device)
        return self.run(emb + pos.unsqueeze(0), mask), emb


class Decoder(_FastformerStack):
    """fastformer.py:71-123"""

    def __init__(self, config):
        super().__init__(config, "decoder")

    def forward(self, enc_seq, mask):
        T = enc_seq.shape[1]
        if not (not self.training and T > self.max_seq_len):
            T = min(T, self.max_seq_len)
            enc_seq, mask = enc_seq[:, :T, :], mask[:, :T]
        pos = self._pos(T, enc_seq.device)
        return self.run(enc_seq + pos.unsqueeze(0), mask), mask


def reset_fastformer_parameters(stack):
    """initialisers of the reference: FastAttention.init_weights - every nn.Linear weight N(0, 0.02), bias 0; torch defaults for the
    Conv1d layers and LayerNorm; nn.Embedding default N(0, 1) with a zero padding row"""
    params = dict(stack.named_parameters())
    for name, p in params.items():
        if name.endswith("position_enc"):
            continue
        if ".0.fn." in name and name.endswith(".weight"):
            nn.init.normal_(p, 0.0, 0.02)
        elif ".0.fn." in name and name.endswith(".bias"):
            nn.init.zeros_(p)
        elif name.endswith("src_word_emb.weight"):
            nn.init.normal_(p)
            with torch.no_grad():
                p[0].zero_()
        elif ".1.fn." in name and name.endswith(".weight"):
            nn.init.kaiming_uniform_(p, a=math.sqrt(5))
        elif ".1.fn." in name and name.endswith(".bias"):
            fan_in = params[name[:-4] + "weight"][0].numel()
            nn.init.uniform_(p, -1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))
        elif name.endswith("norm.weight"):
            nn.init.ones_(p)
        elif name.endswith("norm.bias"):
            nn.init.zeros_(p)
