"""HiFi-GAN generator, inference only, on the gfx950 kernels of csrc/vocoder.hip (include/ctts.h ctts_vocoder_conv / ctts_vocoder_post).

Replaces the reference's `hifigan.Generator` (hifigan/models.py:112-173) where `utils/model.py:42-92` (`get_vocoder`, `vocoder_infer`)
builds and runs it: same constructor (`Generator(h)`, `h` the AttrDict of hifigan/config.json), same module tree and state-dict keys in
both weight forms (weight norm: `*.weight_g` / `*.weight_v` / `*.bias`; after `remove_weight_norm()`: `*.weight` / `*.bias`), so a
released checkpoint's `ckpt["generator"]` loads unchanged.  Like the reference (models.py:121) it always builds type-1 ResBlocks.

`forward(mel [B, 80, T]) -> wav [B, 1, 256 T]` on device tensors only (a CPU tensor raises: there is no CPU path), no autograd graph.
The mel may be the transposed view of the acoustic model's channel-last [B, T, 80] output: the first layer reads it through its strides,
no copy.  Per forward: 1 + num_upsamples + 6 x num_upsamples x num_kernels + 1 launches (78 for V1), every leaky_relu, residual add,
`xs += resblock(x)` and `/ num_kernels` fused into a convolution's load or epilogue.  Arithmetic: kernels.BF16_SPLIT (CTTS_X6=0 = exact
fp32 MFMA; default = the exact three-way bf16 split).  The folded, packed (and split) weights are cached and rebuilt when a parameter
changes (load_state_dict, remove_weight_norm, .to(), in-place edits: version counters + kernels.WEIGHTS_EPOCH).

`forward(mel, lens)` is the length-aware form (include/ctts.h, HiFi-GAN block): `lens` holds one mel-frame count per utterance and
utterance b is vocoded exactly as `forward(mel[b:b + 1, :, :lens[b]])` would vocode it alone, bit for bit - the padded frames are never
read (NaN there is harmless) and the wav holds exact zeros from sample 256 lens[b] on.  lens[b] > T behaves as T; lens[b] == 0 gives an
all-zero row (the reference raises for an empty mel: this is our own definition).  Same launches as the dense forward (tiles beyond an
utterance's end return at once), no host read of `lens`: a captured forward may be replayed with other values in the same tensor.
`infer_wavs` is the ragged counterpart of the reference's `vocoder_infer` (utils/model.py:74-92).

The module call `g(mel, lens=None, precision=None)`: "fp32" (the default) is the path above; "fp16" is the half-precision inference mode on the kernels of
csrc/vocoder_h.hip (include/ctts.h, "fp16 mode": fp16 weights and activations, one v_mfma_f32_32x32x16_f16 term per product, fp32
accumulation, epilogue and conv_post; the wav is fp32 in both modes).  `precision=None` means `self.default_precision`, which the
constructor takes from the environment variable CTTS_VOCODER_PRECISION (unset / "fp32" / "fp16") - the switch of the zero-edit drop-in
route, whose `vocoder_infer` calls `vocoder(mels)`.  Both precisions run the one layer schedule of `_forward`; a precision supplies its
packer and kernels (`_Mode`) and has its own packed-weight cache slot under the same invalidation rules, so the two can be mixed on one
generator in any order.  `forward(mel, lens)` itself keeps the two-argument signature its callers and tests
know and runs the precision of the call in progress (`precision` of `g(...)`, else default_precision); `infer_wavs` keeps its
signature too and follows the generator's default_precision.  `Generator.half()` is not the switch: it converts the parameters as on any nn.Module."""
import collections
import os

import numpy as np
import torch
import torch.nn as nn
from torch.nn import Conv1d, ConvTranspose1d
from torch.nn.utils import remove_weight_norm as _remove_weight_norm

from . import _lib
from . import kernels as K

LRELU_SLOPE = 0.1          # models.py:7
POST_SLOPE = 0.01          # F.leaky_relu's default, models.py:161
PRECISIONS = ("fp32", "fp16")
PRECISION_ENV = "CTTS_VOCODER_PRECISION"


def _check_precision(p, what):
    if p not in PRECISIONS:
        raise ValueError(f"{what}: precision must be one of {PRECISIONS}, got {p!r}")
    return p


# What a precision contributes to the forward: `key` tags its cache slot's key, pack(folded weight, transposed_u) -> the packed-weight
# tuple, conv(x, packed + (bias,), Cin, Cout, k, dil, **epilogue) and post are its kernels.  The layer schedule is Generator._forward's.
_Mode = collections.namedtuple("_Mode", "key pack conv post")


def _mode(precision):
    if precision == "fp16":           # weights folded in fp32, rounded once to fp16; biases and conv_post's weight stay fp32
        return _Mode("fp16", lambda w, u: (K.vocoder_pack_weight_h(w, transposed_u=u),),
                     lambda x, wb, *a, **kw: K.vocoder_conv_h(x, wb[0], *a, bias=wb[1], **kw), K.vocoder_post_h)
    split = K.BF16_SPLIT
    return _Mode(split, lambda w, u: K.vocoder_pack_weight(w, transposed_u=u, planes=split),
                 lambda x, wpb, *a, **kw: K.vocoder_conv(x, wpb[0], wpb[1], *a, bias=wpb[2], bf16_split=split, **kw), K.vocoder_post)


class AttrDict(dict):
    """hifigan/__init__.py's config container: keys readable as attributes."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


def get_padding(kernel_size, dilation=1):
    return int((kernel_size * dilation - dilation) / 2)


def _weight_norm(m):
    # the reference's torch.nn.utils.weight_norm (dim 0: output channels of a Conv1d, INPUT channels of a ConvTranspose1d), whose
    # parameter names a checkpoint carries; its forward pre-hook never runs here (the kernels fold g / v themselves)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        return torch.nn.utils.weight_norm(m)


def _folded_weight(m):
    """effective weight of a (possibly weight-normed) conv: g v / ||v|| over every dim but 0, as WeightNorm.compute_weight"""
    if hasattr(m, "weight_g") and hasattr(m, "weight_v"):
        return torch._weight_norm(m.weight_v, m.weight_g, 0)
    return m.weight


class ResBlock(nn.Module):
    """models.py:18-109 (ResBlock1): three (dilated conv, conv) pairs with a residual each."""

    def __init__(self, h, channels, kernel_size=3, dilation=(1, 3, 5)):
        super().__init__()
        self.h = h
        self.kernel_size = kernel_size
        self.dilation = tuple(dilation[:3])
        self.convs1 = nn.ModuleList([_weight_norm(Conv1d(channels, channels, kernel_size, 1, dilation=d, padding=get_padding(kernel_size, d)))
                                     for d in self.dilation])
        self.convs2 = nn.ModuleList([_weight_norm(Conv1d(channels, channels, kernel_size, 1, dilation=1, padding=get_padding(kernel_size, 1)))
                                     for _ in self.dilation])

    def remove_weight_norm(self):
        for m in self.convs1:
            _remove_weight_norm(m)
        for m in self.convs2:
            _remove_weight_norm(m)


class Generator(nn.Module):
    """models.py:112-173 on the HIP kernels.  Raises NotImplementedError for an upsampler the polyphase kernel does not cover
    (kernel % rate != 0 or kernel - rate odd) or a dilated conv whose halo exceeds 64 rows.
    Accepted: every config with kernel % rate == 0, (kernel - rate) even, kernel / rate <= 65, odd ResBlock kernels with three dilations
    and (kernel - 1) x dilation <= 64 - V1, V2 and the others tests/test_vocoder_contract_gpu.py runs."""

    def __init__(self, h):
        super().__init__()
        self.h = h
        self.num_kernels = len(h.resblock_kernel_sizes)
        self.num_upsamples = len(h.upsample_rates)
        for u, k in zip(h.upsample_rates, h.upsample_kernel_sizes):
            if k % u or (k - u) % 2:
                raise NotImplementedError(f"HiFi-GAN upsampler with rate {u} and kernel {k}: the native ConvTranspose1d needs "
                                          "kernel % rate == 0 and (kernel - rate) even")
            if k // u - 1 > 64:
                raise NotImplementedError(f"HiFi-GAN upsampler kernel {k} / rate {u}: more than 65 taps")
        for k, ds in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
            if k % 2 == 0 or any((k - 1) * d > 64 for d in ds[:3]) or len(ds) < 3:
                raise NotImplementedError(f"HiFi-GAN ResBlock kernel {k} dilations {ds}: the native conv needs an odd kernel, three "
                                          "dilations and (kernel - 1) x dilation <= 64")
        c0 = h.upsample_initial_channel
        self.conv_pre = _weight_norm(Conv1d(80, c0, 7, 1, padding=3))
        self.ups = nn.ModuleList()
        for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
            self.ups.append(_weight_norm(ConvTranspose1d(c0 // (2 ** i), c0 // (2 ** (i + 1)), k, u, padding=(k - u) // 2)))
        self.resblocks = nn.ModuleList()
        ch = c0
        for i in range(len(self.ups)):
            ch = c0 // (2 ** (i + 1))
            for k, d in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
                self.resblocks.append(ResBlock(h, ch, k, d))
        self.conv_post = _weight_norm(Conv1d(ch, 1, 7, 1, padding=3))
        self._packs = {}                                      # precision -> (key, pack): neither mode rebuilds or reads the other's
        self._call_precision = None                           # set by __call__(..., precision=) for the duration of that call
        self.default_precision = _check_precision(os.environ.get(PRECISION_ENV) or "fp32", PRECISION_ENV)

    def remove_weight_norm(self):
        for m in self.ups:
            _remove_weight_norm(m)
        for m in self.resblocks:
            m.remove_weight_norm()
        _remove_weight_norm(self.conv_pre)
        _remove_weight_norm(self.conv_post)

    # ---- packed weights ----------------------------------------------------------------------------------------------------------
    def _key(self, split):
        return (split, K.WEIGHTS_EPOCH[0], tuple((p.data_ptr(), p._version, tuple(p.shape)) for p in self.parameters()))

    def _build_pack(self, pack):
        """(pre, ups, resblocks, post) with every conv as pack(folded weight, transposed_u) + (fp32 bias,); conv_post's weight as fp32
        [k, C].  The one traversal both modes' caches are built by."""
        def conv(m, u=0):
            return tuple(pack(_folded_weight(m), u)) + (m.bias.detach().float().contiguous(),)

        with torch.no_grad():
            pre = conv(self.conv_pre)
            ups = [conv(m, m.stride[0]) for m in self.ups]
            rbs = [[(conv(c1), conv(c2)) for c1, c2 in zip(rb.convs1, rb.convs2)] for rb in self.resblocks]
            wpost = _folded_weight(self.conv_post)[0].detach().float().t().contiguous()        # [k, C]
            post = (wpost, self.conv_post.bias.detach().float().contiguous())
        return (pre, ups, rbs, post)

    def _packed(self, precision, mode):
        """the mode's packed weights from its own cache slot, rebuilt when its key changed"""
        key = self._key(mode.key)
        if precision not in self._packs or self._packs[precision][0] != key:
            self._packs[precision] = (key, self._build_pack(mode.pack))
        return self._packs[precision][1]

    # ---- forward -----------------------------------------------------------------------------------------------------------------
    def __call__(self, x, lens=None, precision=None):
        """the module call with the per-call `precision` ("fp32" / "fp16"; None = self.default_precision): nn.Module's own call (hooks
        included) around forward(x, lens), which reads the precision of the call in progress.  A bad value raises ValueError here.
        forward keeps its (x, lens) signature, so the value travels on the module for the duration of the call: one generator must
        not be called from two threads with different `precision` arguments at once (calls that leave it None are unaffected)."""
        if precision is None:
            return super().__call__(x, lens=lens)
        prev, self._call_precision = self._call_precision, _check_precision(precision, "hifigan Generator")
        try:
            return super().__call__(x, lens=lens)
        finally:
            self._call_precision = prev

    def forward(self, x, lens=None):
        return self._forward(x, lens=lens, precision=self._call_precision)

    @staticmethod
    def _device_lens(lens, x, what="hifigan Generator"):
        """`lens` of forward() -> a contiguous device int32 [B] tensor (`what`: the caller's name, for the messages; melgan.Generator
        shares this).  A device int32 tensor goes in as it is (the kernels clamp it to
        [0, T]); a device int64 tensor (the acoustic model's mel_lens) is clamped and narrowed on the device, no sync; a list or a CPU
        tensor is copied to the device once.  Raises CttsError for a wrong shape or a non-integer dtype, before any launch."""
        B, T = x.shape[0], x.shape[2]
        if not torch.is_tensor(lens):
            try:
                lens = torch.as_tensor(lens)
            except Exception as e:
                raise _lib.CttsError(f"{what}: lens must be a tensor or a list of integers ({e})") from None
        if lens.dtype not in (torch.int32, torch.int64):
            raise _lib.CttsError(f"{what}: lens must be int32 or int64, got {lens.dtype}")
        if tuple(lens.shape) != (B,):
            raise _lib.CttsError(f"{what}: lens must have shape ({B},) for a mel {tuple(x.shape)}, got {tuple(lens.shape)}")
        if lens.device != x.device:
            if lens.is_cuda:
                raise _lib.CttsError(f"{what}: lens is on {lens.device}, the mel on {x.device}")
            lens = lens.to(x.device)
        if lens.dtype == torch.int64:
            lens = lens.clamp(0, T).to(torch.int32)
        return lens.contiguous()

    def _forward(self, x, stage_cb=None, lens=None, precision=None):
        """forward in either precision - the only copy of the layer schedule; stage_cb(name) after conv_pre, each upsampling stage and
        conv_post (tools/bench_vocoder.py's per-stage events)"""
        precision = _check_precision(self.default_precision if precision is None else precision, "hifigan Generator")
        if not x.is_cuda:
            raise _lib.CttsError("hifigan Generator: the mel must be a device (HIP) tensor - there is no CPU path")
        if x.dim() != 3 or x.shape[1] != 80:
            raise _lib.CttsError(f"hifigan Generator: expected mel [B, 80, T], got {tuple(x.shape)}")
        mode = _mode(precision)
        with torch.no_grad():
            if lens is not None:
                lens = self._device_lens(lens, x)
            s = 1                                              # rows per mel frame of the current signal (the kernels' len_mul)
            pre, ups, rbs, post = self._packed(precision, mode)
            xt = x.float().transpose(1, 2)                     # fp32 [B, T, 80] channel-last view (the model's own mel layout); the
            c0 = self.h.upsample_initial_channel               # fp16 mode rounds it when the first layer stages it
            hcur = mode.conv(xt, pre, 80, c0, 7, 1, lens=lens, len_mul=s)                                      # models.py:146
            if stage_cb:
                stage_cb("conv_pre")
            nk = self.num_kernels
            for i in range(self.num_upsamples):
                u, kup = self.h.upsample_rates[i], self.h.upsample_kernel_sizes[i]
                cin, cout = c0 // (2 ** i), c0 // (2 ** (i + 1))
                hcur = mode.conv(hcur, ups[i], cin, cout, kup, 1, transposed_u=u, slope=LRELU_SLOPE, lens=lens,    # models.py:148-149
                                 len_mul=s)
                s *= u
                xs = torch.empty_like(hcur)
                for j in range(nk):                                                                            # models.py:150-158
                    rb = self.resblocks[i * nk + j]
                    k = rb.kernel_size
                    cur = hcur
                    for l, d in enumerate(rb.dilation):                                                         # models.py:96-104
                        c1, c2 = rbs[i * nk + j][l]
                        t = mode.conv(cur, c1, cout, cout, k, d, slope=LRELU_SLOPE, lens=lens, len_mul=s)
                        if l < len(rb.dilation) - 1:
                            cur = mode.conv(t, c2, cout, cout, k, 1, slope=LRELU_SLOPE, R=cur, lens=lens, len_mul=s)
                        else:             # xs = resblock_0(x); xs += resblock_j(x); x = xs / num_kernels - in the epilogue
                            last = j == nk - 1
                            mode.conv(t, c2, cout, cout, k, 1, slope=LRELU_SLOPE, R=cur, out=xs, alpha=1.0 / nk if last else 1.0,
                                      beta=0.0 if j == 0 else (1.0 / nk if last else 1.0), lens=lens, len_mul=s)
                hcur = xs
                if stage_cb:
                    stage_cb(f"stage{i}")
            wpost, bpost = post
            wav = mode.post(hcur, wpost, bpost, POST_SLOPE, lens=lens, len_mul=s)                            # models.py:161-163
            if stage_cb:
                stage_cb("conv_post")
            return wav


def infer_wavs(vocoder, mels, mel_lens, max_wav_value=32768.0):
    """The ragged counterpart of the reference's `vocoder_infer` (utils/model.py:74-92) with its result contract: mels [B, 80, T] on the
    device (the transposed view of the acoustic model's [B, T, 80] output is fine), mel_lens one frame count per utterance (what
    `Generator.forward` takes as `lens`) -> a list of B int16 numpy arrays, `(wav * max_wav_value).astype("int16")` on the host, the
    b-th 256 x min(mel_lens[b], T) samples long (the generator's own hop: the product of its upsample_rates).  Unlike the reference,
    each array is the audio of its utterance vocoded alone: it does not depend on the batch's padding or on the other utterances.
    The arithmetic is the generator's `default_precision` ("fp32" / "fp16": set the attribute, or CTTS_VOCODER_PRECISION)."""
    wavs = vocoder(mels, lens=mel_lens).squeeze(1)
    hop = wavs.shape[1] // mels.shape[2]
    lens = mel_lens.tolist() if torch.is_tensor(mel_lens) else [int(v) for v in mel_lens]
    wavs = (wavs.cpu().numpy() * max_wav_value).astype("int16")
    return [wavs[i][: hop * max(0, min(int(n), mels.shape[2]))] for i, n in enumerate(lens)]


def infer_wavs_loudness(vocoder, mels, mel_lens, loudness=-22.0, sampling_rate=22050, max_wav_value=32768.0):
    """`infer_wavs` with every utterance delivered at `loudness` LUFS: the ragged generator output is brought to that ITU-R BS.1770
    integrated loudness on the device, at `sampling_rate` (`loudness.normalize_loudness` with peak_limit=True: an utterance that would
    clip is scaled to a peak of 1 instead), before the int16 cast on the host.  Every utterance must be at least 0.4 s long.
    `infer_wavs` itself keeps its parameter list: earlier callers and tests pin it."""
    from .loudness import normalize_loudness
    wavs = vocoder(mels, lens=mel_lens).squeeze(1)
    hop = wavs.shape[1] // mels.shape[2]
    lens = mel_lens.tolist() if torch.is_tensor(mel_lens) else [int(v) for v in mel_lens]
    wav_lens = [hop * max(0, min(int(n), mels.shape[2])) for n in lens]
    wavs = normalize_loudness(wavs, wav_lens, sampling_rate, target=float(loudness), peak_limit=True)[0]
    # the peak guard allows a sample of exactly 1.0, which scales to +32768: saturate it (a plain cast would wrap to -32768)
    wavs = np.clip(wavs.cpu().numpy() * max_wav_value, -32768.0, 32767.0).astype("int16")
    return [wavs[i][:n] for i, n in enumerate(wav_lens)]
