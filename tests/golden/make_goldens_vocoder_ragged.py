"""Golden-vector generator for the length-aware HiFi-GAN forward - runs ONLY where the reference checkout exists (needs its hifigan/
package).  Writes data only:
  g20_hifigan_ragged.npz    the g17 fixture's reduced generator and weight-norm weights (read back through tests/hifigan_restate.py
                            load_g17: nothing of them is stored again), a mel batch [4, 80, 32] with lengths [32, 13, 1, 27] whose
                            padded frames are non-zero (-4 +- 0.3, as a PostNet leaves log-mel silence), and the live reference
                            Generator's (hifigan/models.py:112-173) four B = 1 outputs on the UNPADDED mels, concatenated: `wavs`
                            [73 x 256] float32, utterance b at [256 sum(lens[:b]), 256 sum(lens[:b + 1])).  `trim_diff` [4]: max abs
                            difference between the reference's batch-then-trim (utils/model.py:74-92 vocoder_infer) and alone, per
                            utterance - what a length-aware forward changes; `wav_absmax` [4]: each wav's own amplitude.
CPU, float32, one thread, seeded.  Re-run:  python tests/golden/make_goldens_vocoder_ragged.py
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))
from hifigan_restate import load_g17  # noqa: E402
from hifigan import AttrDict, Generator  # noqa: E402  (the reference's own package)

LENS = [32, 13, 1, 27]


def main():
    _, h, sd = load_g17(os.path.join(OUT, "g17_hifigan_small.npz"))
    g = Generator(AttrDict(h)).eval()
    g.load_state_dict(sd)
    gen = torch.Generator().manual_seed(20)
    T = max(LENS)
    mel = torch.randn(len(LENS), 80, T, generator=gen)
    for b, n in enumerate(LENS):
        mel[b, :, n:] = -4.0 + 0.3 * torch.randn(80, T - n, generator=gen)
    with torch.no_grad():
        alone = [g(mel[b:b + 1, :, :n])[0, 0] for b, n in enumerate(LENS)]
        batch = g(mel)[:, 0]
    for b, n in enumerate(LENS):
        assert alone[b].shape == (256 * n,) and torch.isfinite(alone[b]).all()
    trim_diff = np.array([float((batch[b, :256 * n] - alone[b]).abs().max()) for b, n in enumerate(LENS)], dtype=np.float64)
    absmax = np.array([float(w.abs().max()) for w in alone], dtype=np.float64)
    print("batch-then-trim vs alone:", trim_diff, "wav abs max:", absmax)
    np.savez_compressed(os.path.join(OUT, "g20_hifigan_ragged.npz"), mel=mel.numpy(), mel_lens=np.array(LENS, dtype=np.int64),
                        wavs=torch.cat(alone).numpy(), trim_diff=trim_diff, wav_absmax=absmax)
    print("written", os.path.join(OUT, "g20_hifigan_ragged.npz"))


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
