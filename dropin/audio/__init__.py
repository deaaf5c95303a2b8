"""Shadow of the reference's `audio` package (its `audio/`): `import audio as Audio; Audio.stft.TacotronSTFT(...)`,
`Audio.tools.get_mel_from_wav(wav, stft)` as `preprocessor/preprocessor.py:38-46,232` uses them (the HIP mel kernel), and the Griffin-Lim
helpers `audio.stft.STFT`, `audio.audio_processing.griffin_lim` / `window_sumsquare` / `dynamic_range_*` and
`audio.tools.inv_mel_spec` (csrc/griffinlim.hip; inv_mel_spec reads `_stft.stft_fn` - the reference's `_stft._stft_fn` does not exist)."""
import os
import sys

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _REPO not in sys.path:
    sys.path.insert(0, _REPO)

from . import audio_processing, stft, tools  # noqa: E402,F401
