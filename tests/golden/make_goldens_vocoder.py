"""Golden-vector generator for the HiFi-GAN vocoder - runs ONLY where the reference checkout exists (needs its hifigan/ package).

Runs the live reference Generator (hifigan/models.py:112-173) on CPU in float32, seeded and deterministic, and writes data only:
  g17_hifigan_small.npz                 reduced config (upsample_initial_channel 64, V1's rates / kernels / dilations), weight-norm
                                        weights scaled so that the signals are O(0.1 - 1): every `weight_g` and bias as data, every
                                        `weight_v` in closed form (tests/hifigan_restate.py g17_weight_v: a keyed hash, only its shape is
                                        stored - the fixture stays small), a ragged B = 2 mel batch (T = 32 and 13, non-zero padding),
                                        the wav before and after remove_weight_norm() (the latter as its difference from the former);
                                        tests/hifigan_restate.py load_g17 reads it back
  state_dict_schema_hifigan_v1.json     key -> shape of the V1 generator in both weight forms
Re-run:  python tests/golden/make_goldens_vocoder.py
"""
import json
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))
from hifigan_restate import g17_weight_v  # noqa: E402
from hifigan import AttrDict, Generator  # noqa: E402  (the reference's own package)

V1 = dict(upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], resblock="1")


def schema():
    torch.manual_seed(0)
    g = Generator(AttrDict(V1))
    wn = {k: list(v.shape) for k, v in g.state_dict().items()}
    g.remove_weight_norm()
    folded = {k: list(v.shape) for k, v in g.state_dict().items()}
    return {"weight_norm": wn, "folded": folded,
            "weight_norm_numel": int(sum(np.prod(s) for s in wn.values())), "folded_numel": int(sum(np.prod(s) for s in folded.values()))}


def small():
    h = dict(V1, upsample_initial_channel=64)
    torch.manual_seed(1234)
    g = Generator(AttrDict(h)).eval()
    gen = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for name, m in g.named_modules():
            if not hasattr(m, "weight_g"):
                continue
            m.weight_v.copy_(g17_weight_v(name, m.weight_v.shape))
            # per-filter norm g: ~1 keeps a Conv1d's scale; a ConvTranspose1d (norm over its Cin dim-0 slices) needs ~sqrt(u Cout / Cin)
            gain = 1.0
            if name.startswith("ups."):
                gain = (m.stride[0] * m.out_channels / m.in_channels) ** 0.5
            elif name == "conv_post":
                gain = 0.5
            m.weight_g.copy_(gain * (0.75 + 0.5 * torch.rand(m.weight_g.shape, generator=gen)))
            m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=gen))
    mel = torch.randn(2, 80, 32, generator=gen)
    mel[1, :, 13:] = -4.0 + 0.3 * torch.randn(80, 19, generator=gen)        # padding of the short utterance, non-zero
    lens = np.array([32, 13], dtype=np.int64)
    sd = {k: v.detach().clone() for k, v in g.state_dict().items()}
    with torch.no_grad():
        wav_wn = g(mel)
        g.remove_weight_norm()
        wav_folded = g(mel)
    print("wav std", float(wav_wn.std()), "max", float(wav_wn.abs().max()))
    arrays = {"sd/" + k: v.numpy() for k, v in sd.items() if not k.endswith(".weight_v")}
    for k, v in sd.items():
        if k.endswith(".weight_v"):
            assert torch.equal(v, g17_weight_v(k[:-len(".weight_v")], v.shape))
            arrays["vshape/" + k[:-len(".weight_v")]] = np.array(v.shape, dtype=np.int64)
    # the folded wav as its difference from the weight-norm wav (zero when the two forms agree bit for bit): half the bytes
    diff = wav_folded.numpy() - wav_wn.numpy()
    assert np.array_equal(wav_wn.numpy() + diff, wav_folded.numpy())
    arrays.update(mel=mel.numpy(), mel_lens=lens, wav_wn=wav_wn.numpy(), wav_folded_minus_wn=diff,
                  config=np.frombuffer(json.dumps(h).encode(), dtype=np.uint8))
    np.savez_compressed(os.path.join(OUT, "g17_hifigan_small.npz"), **arrays)


if __name__ == "__main__":
    torch.set_num_threads(1)
    with open(os.path.join(OUT, "state_dict_schema_hifigan_v1.json"), "w") as f:
        json.dump(schema(), f, indent=0, sort_keys=True)
    small()
    print("written", OUT)
