"""The MelGAN generator (descriptinc/melgan-neurips mel2wav/modules.py, restated from its published layout) in plain torch, twice:

  generator_forward   a functional restatement on folded weights (F.pad(mode="reflect"), F.conv1d, F.conv_transpose1d) - the oracle of
                      the MelGAN tests (run in float64) and the stock-torch fp32 baseline of tools/bench_melgan.py;
  stock_generator     an independent nn.Sequential build of the module table with torch's own weight_norm, whose state dict gives the
                      checkpoint keys (tests/golden/melgan_state_dict_schema.json) and whose forward the restatement is checked against.

Neither imports the package.  Also here: the random-weight recipe of the tests and the benchmark, and the FLOP count."""
import os
import sys
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hifigan_restate import fold_state_dict  # noqa: E402,F401  (prefix -> (weight, bias), weight norm folded)

SLOPE = 0.2
RATIOS = (8, 8, 2, 2)
N_RES = 3


def _reflect_conv(x, wb, pad, dil=1):
    return F.conv1d(F.pad(x, (pad, pad), mode="reflect"), wb[0], wb[1], dilation=dil)


def generator_forward(W, x, stage_cb=None):
    """the forward of the module table on folded weights W (fold_state_dict); x [B, 80, T] in W's dtype, T >= 4"""
    x = _reflect_conv(x, W["model.1"], 3)
    if stage_cb:
        stage_cb("conv_pre")
    i = 2
    for s, r in enumerate(RATIOS):
        w, b = W[f"model.{i + 1}"]
        x = F.conv_transpose1d(F.leaky_relu(x, SLOPE), w, b, stride=r, padding=r // 2 + r % 2, output_padding=r % 2)
        for j in range(N_RES):
            p = f"model.{i + 2 + j}"
            t = _reflect_conv(F.leaky_relu(x, SLOPE), W[p + ".block.2"], 3 ** j, 3 ** j)
            t = F.conv1d(F.leaky_relu(t, SLOPE), *W[p + ".block.4"])
            x = F.conv1d(x, *W[p + ".shortcut"]) + t
        i += 2 + N_RES
        if stage_cb:
            stage_cb(f"stage{s}")
    x = torch.tanh(_reflect_conv(F.leaky_relu(x, SLOPE), W[f"model.{i + 2}"], 3))
    if stage_cb:
        stage_cb("conv_post")
    return x


def _wn(m):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        return torch.nn.utils.weight_norm(m)


class _ResnetBlock(nn.Module):
    def __init__(self, dim, dilation):
        super().__init__()
        self.block = nn.Sequential(nn.LeakyReLU(SLOPE), nn.ReflectionPad1d(dilation), _wn(nn.Conv1d(dim, dim, 3, dilation=dilation)),
                                   nn.LeakyReLU(SLOPE), _wn(nn.Conv1d(dim, dim, 1)))
        self.shortcut = _wn(nn.Conv1d(dim, dim, 1))

    def forward(self, x):
        return self.shortcut(x) + self.block(x)


class _Stock(nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model(x)


def stock_generator(input_size=80, ngf=32):
    """the module table as stock torch modules (this one IS called: forward = model(x))"""
    c = 16 * ngf
    model = [nn.ReflectionPad1d(3), _wn(nn.Conv1d(input_size, c, 7))]
    for r in RATIOS:
        model += [nn.LeakyReLU(SLOPE), _wn(nn.ConvTranspose1d(c, c // 2, 2 * r, stride=r, padding=r // 2 + r % 2, output_padding=r % 2))]
        model += [_ResnetBlock(c // 2, 3 ** j) for j in range(N_RES)]
        c //= 2
    model += [nn.LeakyReLU(SLOPE), nn.ReflectionPad1d(3), _wn(nn.Conv1d(ngf, 1, 7)), nn.Tanh()]
    return _Stock(nn.Sequential(*model))


def recipe_(module, seed=11):
    """the random weights of the tests and the benchmark, written into a weight-normed generator in place: weight_v ~ N(0, 1),
    weight_g = gain U(0.75, 1.25) with gain sqrt(stride) for the upsamplers, 0.5 for the last conv and 0.9 otherwise,
    bias ~ 0.05 N(0, 1).  -> module (wav std about 0.2, peak about 0.75: the tanh is exercised)"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if hasattr(m, "weight_g"):
                m.weight_v.copy_(torch.randn(m.weight_v.shape, generator=gen))
                gain = m.stride[0] ** 0.5 if isinstance(m, nn.ConvTranspose1d) else (0.5 if m.out_channels == 1 else 0.9)
                m.weight_g.copy_(gain * (0.75 + 0.5 * torch.rand(m.weight_g.shape, generator=gen)))
                m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=gen))
    return module


def recipe_state_dict(seed=11):
    return {k: v.detach().clone() for k, v in recipe_(stock_generator(), seed).state_dict().items()}


def flops_per_frame(input_size=80, ngf=32):
    """algorithmic FLOP (multiply-add = 2) of one mel frame through the generator, counted as hifigan_restate.flops_per_frame"""
    c = 16 * ngf
    f = 2 * input_size * c * 7
    rate = 1
    for r in RATIOS:
        f += 2 * rate * c * (c // 2) * 2 * r
        rate *= r
        c //= 2
        f += rate * N_RES * (2 * c * c * 3 + 2 * c * c + 2 * c * c)
    return f + 2 * rate * c * 7
