"""Shadow of the reference's `hifigan` package (`hifigan/__init__.py`, `hifigan/models.py:112-173`): with `dropin/` in front of the
reference checkout on `sys.path`, the reference's UNMODIFIED `utils/model.py:42-92` (`import hifigan`; `get_vocoder` builds
`hifigan.Generator(hifigan.AttrDict(config))`, loads `ckpt["generator"]`, calls `remove_weight_norm()`; `vocoder_infer` runs it)
and therefore `synthesize.py`, `train.py` and `evaluate.py` synthesise on the native HIP vocoder.  `hifigan/config.json` and the
checkpoints are opened relative to the working directory by the caller, so they are untouched.

    PYTHONPATH=<repo>/dropin:<repo>  python synthesize.py --source ... --restore_step ... --mode batch -p ... -m ... -t ...
"""
import os
import sys

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _REPO not in sys.path:
    sys.path.insert(0, _REPO)

import ctts_amd  # noqa: E402,F401
from ctts_amd.vocoder import AttrDict, Generator  # noqa: E402,F401

__all__ = ["AttrDict", "Generator"]
