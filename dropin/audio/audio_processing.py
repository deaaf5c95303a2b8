"""`audio.audio_processing` (the reference's `audio/audio_processing.py:7-100`) -> ctts_amd.audio: griffin_lim on csrc/griffinlim.hip,
window_sumsquare (host numpy, like the reference) and dynamic_range_compression / decompression"""
from ctts_amd.audio import (dynamic_range_compression, dynamic_range_decompression, griffin_lim,  # noqa: F401
                            window_sumsquare)
