"""`audio.stft.TacotronSTFT` / `audio.stft.STFT` (the reference's `audio/stft.py:22-185`) -> ctts_amd.audio (csrc/mel.hip, csrc/griffinlim.hip)"""
from ctts_amd.audio import STFT, TacotronSTFT  # noqa: F401
