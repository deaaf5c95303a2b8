"""`audio.tools.get_mel_from_wav` / `inv_mel_spec` (the reference's `audio/tools.py:8-34`) -> ctts_amd.audio"""
from ctts_amd.audio import get_mel_from_wav, inv_mel_spec  # noqa: F401
