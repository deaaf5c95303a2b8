"""Golden-vector generator for the Griffin-Lim vocoder - runs ONLY where the reference checkout exists (through oracle/ref_import.py).

Runs the live reference audio.stft.STFT / audio.audio_processing.griffin_lim / audio.tools.inv_mel_spec on CPU in float32 and writes
OUTPUTS only; the inputs are regenerated from numpy seeds by tests/griffinlim_restate.py (g19_*):
  g19_griffinlim.npz   tr_mag / tr_phase       STFT.transform of g19_signal() [1, 4000] (16 frames)
                       inv_F{4,5,87}           STFT.inverse of g19_inverse_inputs(F)
                       gl_{0,1,4,60}           griffin_lim(g19_gl_magnitude(), stft, n) after np.random.seed(GL_SEED)
                       invmel_wav              inv_mel_spec(g19_mel(), tmp.wav, TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)) after
                                               np.random.seed(INVMEL_SEED), read back from the wav (the reference reads `_stft._stft_fn`;
                                               the attribute is `stft_fn` - aliased here)
                       drift_rel_l2_{n}, drift_max_abs_60: the reference's own float32 Griffin-Lim against a float64 copy of the same
                                               module (same bases, same angles)
librosa is absent: ref_import stubs it, and this generator adds librosa.util.normalize (norm=None returns its input, the only use).
Re-run:  python tests/golden/make_goldens_griffinlim.py
"""
import copy
import os
import sys
import tempfile

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(OUT))
import griffinlim_restate as R  # noqa: E402
from oracle import ref_import  # noqa: E402


def _normalize(S, norm=np.inf, axis=0, threshold=None, fill=None):
    if norm is None:
        return S
    raise NotImplementedError("only norm=None is used by audio_processing.window_sumsquare")


def main():
    ref_import.install()
    sys.modules["librosa.util"].normalize = _normalize
    from audio.stft import STFT, TacotronSTFT
    from audio.audio_processing import griffin_lim
    from audio.tools import inv_mel_spec
    from scipy.io.wavfile import read

    torch.set_num_threads(1)
    stft = STFT(1024, 256, 1024)
    arrays = {}
    with torch.no_grad():
        mag, phase = stft.transform(torch.from_numpy(R.g19_signal()))
        arrays.update(tr_mag=mag.numpy(), tr_phase=phase.numpy())
        for F in R.INV_FRAMES:
            m, p = R.g19_inverse_inputs(F)
            arrays[f"inv_F{F}"] = stft.inverse(torch.from_numpy(m), torch.from_numpy(p)).numpy()
        stft64 = copy.deepcopy(stft).double()
        mag = torch.from_numpy(R.g19_gl_magnitude())
        for n in R.GL_ITERS:
            np.random.seed(R.GL_SEED)
            out = griffin_lim(mag, stft, n).numpy()
            np.random.seed(R.GL_SEED)
            out64 = griffin_lim(mag.double(), stft64, n).numpy()
            arrays[f"gl_{n}"] = out
            arrays[f"drift_rel_l2_{n}"] = np.float64(R.rel_l2(out, out64))
            print(f"gl {n}: fp32 vs fp64 rel-L2 {arrays[f'drift_rel_l2_{n}']:.3g}, max |x| {np.abs(out).max():.3g}")
        arrays["drift_max_abs_60"] = np.float64(np.abs(arrays["gl_60"] - out64).max())
        tac = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
        tac._stft_fn = tac.stft_fn                     # the reference's typo (tools.py:30)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "g19.wav")
            np.random.seed(R.INVMEL_SEED)
            inv_mel_spec(torch.from_numpy(R.g19_mel()), path, tac, 60)
            sr, wav = read(path)
        assert sr == 22050 and wav.dtype == np.float32
        arrays["invmel_wav"] = wav
    np.savez_compressed(os.path.join(OUT, "g19_griffinlim.npz"), **arrays)
    print("written", os.path.join(OUT, "g19_griffinlim.npz"), os.path.getsize(os.path.join(OUT, "g19_griffinlim.npz")), "bytes")


if __name__ == "__main__":
    main()
