"""Functional restatement of the reference HiFi-GAN generator (hifigan/models.py:112-173) in plain torch - the per-shape oracle of the
vocoder tests (run in float64) and the stock-torch fp32 baseline of tools/bench_vocoder.py (F.conv1d / F.conv_transpose1d on the
same folded weights).  It reads a state dict in either form: weight norm (`*.weight_g`, `*.weight_v`) is folded exactly as
torch.nn.utils.weight_norm computes it (dim 0), then everything runs in `dtype` on the tensors' device."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.weights import _hash_uniform  # noqa: E402

LRELU_SLOPE = 0.1                                   # models.py:7


def _get_padding(k, d=1):                           # models.py:15-16
    return int((k * d - d) / 2)


def fold_state_dict(sd, dtype=torch.float64, device=None):
    """-> {prefix: (weight, bias)} with weight-norm pairs folded: w = g v / ||v|| (norm over every dim but 0)."""
    out = {}
    prefixes = sorted({k.rsplit(".", 1)[0] for k in sd})
    for p in prefixes:
        b = sd[p + ".bias"]
        if p + ".weight_g" in sd:
            g, v = sd[p + ".weight_g"].to(dtype), sd[p + ".weight_v"].to(dtype)
            w = torch._weight_norm(v, g, 0)
        else:
            w = sd[p + ".weight"].to(dtype)
        out[p] = (w.to(device) if device is not None else w, (b.to(dtype).to(device) if device is not None else b.to(dtype)))
    return out


def resblock_forward(W, prefix, x, k, dil):         # models.py:96-104 (ResBlock1.forward)
    for l, d in enumerate(dil[:3]):
        w1, b1 = W[f"{prefix}.convs1.{l}"]
        w2, b2 = W[f"{prefix}.convs2.{l}"]
        xt = F.leaky_relu(x, LRELU_SLOPE)
        xt = F.conv1d(xt, w1, b1, 1, _get_padding(k, d), d)
        xt = F.leaky_relu(xt, LRELU_SLOPE)
        xt = F.conv1d(xt, w2, b2, 1, _get_padding(k, 1), 1)
        x = xt + x
    return x


def generator_forward(W, h, x, stage_cb=None):
    """models.py:145-165 on folded weights W (fold_state_dict); x [B, 80, T] in W's dtype.  stage_cb(name) after each stage."""
    nk = len(h["resblock_kernel_sizes"])
    w, b = W["conv_pre"]
    x = F.conv1d(x, w, b, 1, 3)
    if stage_cb:
        stage_cb("conv_pre")
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, LRELU_SLOPE)
        w, b = W[f"ups.{i}"]
        x = F.conv_transpose1d(x, w, b, u, (k - u) // 2)
        xs = None
        for j, (kr, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            r = resblock_forward(W, f"resblocks.{i * nk + j}", x, kr, dil)
            xs = r if xs is None else xs + r
        x = xs / nk
        if stage_cb:
            stage_cb(f"stage{i}")
    x = F.leaky_relu(x)                             # default slope 0.01 (models.py:161)
    w, b = W["conv_post"]
    x = torch.tanh(F.conv1d(x, w, b, 1, 3))
    if stage_cb:
        stage_cb("conv_post")
    return x


def g17_weight_v(name, shape):
    """closed-form `weight_v` of layer `name` in the g17 fixture: uniform [-1, 1) from a keyed hash (oracle/weights.py), so the fixture
    stores only the per-filter norms `weight_g` and the biases - the weight-norm layer normalises v anyway"""
    n = int(np.prod(shape))
    return torch.from_numpy(_hash_uniform("g17." + name + ".weight_v", n).reshape(tuple(shape))).float()


def load_g17(path):
    """-> (npz, config dict, weight-norm state dict) of tests/golden/g17_hifigan_small.npz (make_goldens_vocoder.py)"""
    z = dict(np.load(path))
    z["wav_folded"] = z["wav_wn"] + z.pop("wav_folded_minus_wn")
    h = json.loads(bytes(z["config"]).decode())
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z if k.startswith("sd/")}
    for k in list(z):
        if k.startswith("vshape/"):
            name = k[len("vshape/"):]
            sd[name + ".weight_v"] = g17_weight_v(name, z[k])
    return z, h, sd


def flops_per_frame(h, n_mel=80):
    """algorithmic FLOP (multiply-add = 2) of one mel frame through the generator"""
    c0 = h["upsample_initial_channel"]
    f = 2 * n_mel * c0 * 7
    rate = 1
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        cin, cout = c0 // 2 ** i, c0 // 2 ** (i + 1)
        f += 2 * rate * cin * cout * k              # each input frame feeds k outputs per (cin, cout)
        rate *= u
        for kr, dil in zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]):
            f += rate * len(dil[:3]) * 2 * (2 * cout * cout * kr)
    f += 2 * rate * (c0 // 2 ** len(h["upsample_rates"])) * 7
    return f
