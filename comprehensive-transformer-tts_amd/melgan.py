"""MelGAN generator, inference only, on the gfx950 kernels of csrc/vocoder.hip (include/ctts.h, MelGAN block).

The reference offers `vocoder.model: "MelGAN"` beside HiFi-GAN (utils/model.py:42-92) and gets it from
`torch.hub.load("descriptinc/melgan-neurips", "load_melgan", ...)`: an object with `.mel2wav` (the generator) and `.inverse(mel)`.
This module restates that generator (mel2wav/modules.py) from its published layout: `Generator(input_size=80, ngf=32,
n_residual_layers=3)` holds one `nn.Sequential` named `model` whose indices the checkpoint keys carry -

    0, 1     ReflectionPad1d(3), Conv1d(80, 512, 7)
    per ratio r in (8, 8, 2, 2), channels c -> c / 2 from 512:
             LeakyReLU(0.2), ConvTranspose1d(c, c / 2, 2 r, stride r, padding r // 2 + r % 2, output_padding r % 2),
             3 x ResnetBlock(c / 2, dilation 3 ** j)                                       (indices 2-6, 7-11, 12-16, 17-21)
    22 - 25  LeakyReLU(0.2), ReflectionPad1d(3), Conv1d(32, 1, 7), Tanh

with `ResnetBlock(dim, d)`: `block = [LeakyReLU(0.2), ReflectionPad1d(d), Conv1d(dim, dim, 3, dilation=d), LeakyReLU(0.2),
Conv1d(dim, dim, 1)]`, `shortcut = Conv1d(dim, dim, 1)`, `forward = shortcut(x) + block(x)`; every conv weight-normed.  126
state-dict entries, 4,266,050 parameters.  Both weight forms load (weight norm: `*.weight_g` / `*.weight_v` / `*.bias`; after
`remove_weight_norm()`: `*.weight` / `*.bias`).  No released checkpoint and no copy of that repository was at hand when this was
written: the layout is pinned by tests/golden/melgan_state_dict_schema.json and the arithmetic by a float64 restatement
(tests/melgan_restate.py), parity with a released checkpoint is NOT pinned.

`forward(mel [B, 80, T], lens=None) -> wav [B, 1, 256 T]` on device tensors only, no autograd graph; the mel may be the transposed
view of a channel-last [B, T, 80] tensor (read through its strides).  30 launches: the first conv (reflect-padded), 4 polyphase
ConvTranspose1d, per ResnetBlock the dilated reflect-padded conv and ONE two-operand 1x1 GEMM for `shortcut(x) + block.4(...)`
(K = 2 dim, bias = the sum of both), and the reflect-padded last conv with its tanh.  Arithmetic: kernels.BF16_SPLIT, as HiFi-GAN.
The folded, packed (and split) weights are cached under vocoder.Generator's rules (parameter versions + kernels.WEIGHTS_EPOCH).

Lengths: ReflectionPad1d(3) needs T >= 4 (torch raises below that), so a dense T < 4 raises CttsError before any launch.  With
`lens` (one mel-frame count per utterance) utterance b is vocoded exactly as `forward(mel[b:b + 1, :, :lens[b]])` would vocode it
alone, bit for bit - every reflection happens at the utterance's own end, padded frames are never read - and the wav holds exact
zeros from sample 256 lens[b] on; an utterance shorter than 4 frames (0 included) gives an all-zero row (our own definition),
decided on the device: no host read of `lens`.

`MelVocoder(generator)` is the hub object's synthesis half (`.mel2wav`, `.inverse(mel)`), what the reference's `vocoder_infer`
calls as `vocoder.inverse(mels / np.log(10))`; `load_melgan(path_or_state_dict, device)` builds one from a generator state dict
without the hub.  `infer_wavs` is the ragged counterpart of `vocoder_infer`.  The analysis half (`Audio2Mel`, `vocoder(audio)`)
is not provided."""
import math

import torch
import torch.nn as nn
from torch.nn.utils import remove_weight_norm as _remove_weight_norm

from . import _lib
from . import kernels as K
from .vocoder import Generator as _HifiGenerator, _folded_weight, _weight_norm

SLOPE = 0.2
RATIOS = (8, 8, 2, 2)
HOP = 256                  # the product of RATIOS
MIN_FRAMES = 4             # ReflectionPad1d(3) in front of the first conv


def WNConv1d(*args, **kwargs):
    return _weight_norm(nn.Conv1d(*args, **kwargs))


def WNConvTranspose1d(*args, **kwargs):
    return _weight_norm(nn.ConvTranspose1d(*args, **kwargs))


class ResnetBlock(nn.Module):
    def __init__(self, dim, dilation=1):
        super().__init__()
        self.dilation = dilation
        self.block = nn.Sequential(nn.LeakyReLU(SLOPE), nn.ReflectionPad1d(dilation), WNConv1d(dim, dim, kernel_size=3, dilation=dilation),
                                   nn.LeakyReLU(SLOPE), WNConv1d(dim, dim, kernel_size=1))
        self.shortcut = WNConv1d(dim, dim, kernel_size=1)


class Generator(nn.Module):
    """mel2wav/modules.py's Generator on the HIP kernels (module docstring).  The modules of `model` hold the parameters and give the
    state dict its keys; they are never called."""

    def __init__(self, input_size=80, ngf=32, n_residual_layers=3):
        super().__init__()
        self.input_size, self.ngf, self.n_residual_layers = input_size, ngf, n_residual_layers
        mult = 2 ** len(RATIOS)
        model = [nn.ReflectionPad1d(3), WNConv1d(input_size, mult * ngf, kernel_size=7, padding=0)]
        for r in RATIOS:
            model += [nn.LeakyReLU(SLOPE), WNConvTranspose1d(mult * ngf, mult * ngf // 2, kernel_size=r * 2, stride=r,
                                                             padding=r // 2 + r % 2, output_padding=r % 2)]
            model += [ResnetBlock(mult * ngf // 2, dilation=3 ** j) for j in range(n_residual_layers)]
            mult //= 2
        model += [nn.LeakyReLU(SLOPE), nn.ReflectionPad1d(3), WNConv1d(ngf, 1, kernel_size=7, padding=0), nn.Tanh()]
        self.model = nn.Sequential(*model)
        if 2 * 3 ** (n_residual_layers - 1) > 64:
            raise NotImplementedError(f"MelGAN with {n_residual_layers} residual layers: the native conv needs 2 x dilation <= 64")
        self._packs = {}                                      # tail form -> (key, pack)

    def _convs(self):
        return [m for m in self.model.modules() if isinstance(m, (nn.Conv1d, nn.ConvTranspose1d))]

    def remove_weight_norm(self):
        for m in self._convs():
            _remove_weight_norm(m)

    # ---- packed weights ----------------------------------------------------------------------------------------------------------
    def _key(self, split):
        return (split, K.WEIGHTS_EPOCH[0], tuple((p.data_ptr(), p._version, tuple(p.shape)) for p in self.parameters()))

    def _build_pack(self, split, fused):
        """(pre, [(up, [(conv3, tail), ...]), ...], post): every conv as (w, w_planes, fp32 bias).  fused: a block's tail is the
        two-operand pack [W_block.4 | W_shortcut] with the summed bias; otherwise the pair (shortcut, block.4) of the three-launch form
        (tools/bench_melgan.py's comparison)."""
        def conv(m, u=0):
            return K.vocoder_pack_weight(_folded_weight(m), transposed_u=u, planes=split) + (m.bias.detach().float().contiguous(),)

        def tail(rb):
            if not fused:
                return conv(rb.shortcut), conv(rb.block[4])
            return K.vocoder_pack_weight(_folded_weight(rb.block[4]), planes=split, weight2=_folded_weight(rb.shortcut)) + \
                ((rb.block[4].bias.detach().float() + rb.shortcut.bias.detach().float()).contiguous(),)

        with torch.no_grad():
            mods = list(self.model)
            pre = conv(mods[1])
            stages, i = [], 2
            for r in RATIOS:
                blocks = mods[i + 2: i + 2 + self.n_residual_layers]
                stages.append((conv(mods[i + 1], r), [(conv(rb.block[2]), tail(rb)) for rb in blocks]))
                i += 2 + self.n_residual_layers
            last = mods[i + 2]
            post = (_folded_weight(last)[0].detach().float().t().contiguous(), last.bias.detach().float().contiguous())     # [k, C]
        return pre, stages, post

    def _packed(self, fused):
        split = K.BF16_SPLIT
        key = self._key(split)
        if fused not in self._packs or self._packs[fused][0] != key:
            self._packs[fused] = (key, self._build_pack(split, fused))
        return self._packs[fused][1]

    # ---- forward -----------------------------------------------------------------------------------------------------------------
    def forward(self, x, lens=None):
        return self._forward(x, lens=lens)

    def _forward(self, x, stage_cb=None, lens=None, fused_tail=True):
        """the layer schedule; stage_cb(name) after the first conv, each upsampling stage and the last conv (tools/bench_melgan.py's
        per-stage events).  fused_tail=False runs a block's tail as the shortcut launch followed by block.4 with R= (three launches per
        block): the form the two-operand tail was measured against, kept for that measurement only."""
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != self.input_size:
            raise _lib.CttsError(f"melgan Generator: expected mel [B, {self.input_size}, T], got {tuple(getattr(x, 'shape', ()))}")
        if lens is None and x.shape[2] < MIN_FRAMES:
            raise _lib.CttsError(f"melgan Generator: a mel of {x.shape[2]} frames is shorter than the reflection padding needs (at least "
                                 f"{MIN_FRAMES} frames)")
        if not x.is_cuda:
            raise _lib.CttsError("melgan Generator: the mel must be a device (HIP) tensor - there is no CPU path")
        split = K.BF16_SPLIT

        def conv(inp, wpb, cin, cout, k, dil=1, **kw):
            return K.vocoder_conv(inp, wpb[0], wpb[1], cin, cout, k, dil, bias=wpb[2], bf16_split=split, lens=lens, len_mul=s, **kw)

        with torch.no_grad():
            if lens is not None:
                lens = _HifiGenerator._device_lens(lens, x, "melgan Generator")
                if x.shape[2] < MIN_FRAMES:                    # every utterance is too short to reflect: all-zero rows, no launch
                    return torch.zeros(x.shape[0], 1, HOP * x.shape[2], dtype=torch.float32, device=x.device)
                lens = torch.where(lens >= MIN_FRAMES, lens, torch.zeros_like(lens))      # too short: an empty utterance
            s = 1                                              # rows per mel frame of the current signal (the kernels' len_mul)
            pre, stages, post = self._packed(bool(fused_tail))
            c = 2 ** len(RATIOS) * self.ngf
            h = conv(x.float().transpose(1, 2), pre, self.input_size, c, 7, pad_mode="reflect")
            if stage_cb:
                stage_cb("conv_pre")
            for i, (r, (up, blocks)) in enumerate(zip(RATIOS, stages)):
                h = conv(h, up, c, c // 2, 2 * r, transposed_u=r, slope=SLOPE)
                s *= r
                c //= 2
                for j, (c3, tail) in enumerate(blocks):
                    t = conv(h, c3, c, c, 3, 3 ** j, slope=SLOPE, pad_mode="reflect")
                    if fused_tail:
                        h = conv(t, tail, c, c, 1, slope=SLOPE, x2=h)
                    else:
                        h = conv(t, tail[1], c, c, 1, slope=SLOPE, R=conv(h, tail[0], c, c, 1))
                if stage_cb:
                    stage_cb(f"stage{i}")
            wav = K.vocoder_post(h, post[0], post[1], SLOPE, lens=lens, len_mul=s, pad_mode="reflect")
            if stage_cb:
                stage_cb("conv_post")
            return wav


class MelVocoder:
    """The synthesis half of the hub's `MelVocoder`: `.mel2wav` is the generator, `.inverse(mel)` its waveform [B, 256 T] for a mel
    [B, 80, T] in the log10 scale of that repository (the reference divides its natural-log mel by ln 10 before the call)."""

    def __init__(self, generator):
        self.mel2wav = generator

    def inverse(self, mel):
        return self.mel2wav(mel).squeeze(1)


def load_melgan(path_or_state_dict, device="cuda"):
    """-> MelVocoder around a Generator holding the generator state dict in `path_or_state_dict` (a dict, or the path of a torch.save'd
    one; either weight form), in eval mode on `device`.  The stand-in for `torch.hub.load("descriptinc/melgan-neurips", "load_melgan", ...)`."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        sd = torch.load(sd, map_location="cpu")
    g = Generator()
    if not any(k.endswith(".weight_g") for k in sd):
        g.remove_weight_norm()
    g.load_state_dict(sd)
    return MelVocoder(g.eval().to(device))


def infer_wavs(vocoder, mels, mel_lens, max_wav_value=32768.0):
    """The ragged counterpart of the reference's `vocoder_infer` (utils/model.py:74-92) for `vocoder.model: "MelGAN"`, with
    `vocoder.infer_wavs`' result contract: mels [B, 80, T] on the device in the acoustic model's natural-log scale (divided by ln 10
    here, as the reference does), mel_lens one frame count per utterance -> a list of B int16 numpy arrays,
    `(wav * max_wav_value).astype("int16")` on the host, the b-th 256 x min(mel_lens[b], T) samples long, each the audio of its
    utterance vocoded alone.  `vocoder`: a MelVocoder (or a Generator)."""
    g = getattr(vocoder, "mel2wav", vocoder)
    wavs = g(mels / math.log(10), lens=mel_lens).squeeze(1)
    lens = mel_lens.tolist() if torch.is_tensor(mel_lens) else [int(v) for v in mel_lens]
    wavs = (wavs.cpu().numpy() * max_wav_value).astype("int16")
    return [wavs[i][: HOP * max(0, min(int(n), mels.shape[2]))] for i, n in enumerate(lens)]
