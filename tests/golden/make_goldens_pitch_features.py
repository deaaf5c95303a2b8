"""Golden-vector generator for the pitch target chain - runs ONLY where the reference checkout exists (through oracle/ref_import.py).

Runs the live reference's own numpy code (utils/pitch_tools.py, preprocessor/preprocessor.py:612-618) in float64 on the hand-made f0
tracks of tests/pitch_restate.py FIXTURE_TRACKS (at most 64 frames: leading / trailing unvoiced runs, a repeated first / last value,
a single voiced frame, all unvoiced) and writes, per track `k`, into tests/golden/g19_pitch_chain.npz (data only):
  {k}_f0                      the input track
  {k}_ccf0_uv, {k}_ccf0       convert_continuos_f0(f0)
  {k}_lf0_uv, {k}_lf0         get_cont_lf0(f0)
  {k}_nif0, {k}_nif0_uv       norm_interp_f0(f0, {pitch_norm: log, pitch_norm_eps: 1e-9, use_uv: True})
  {k}_mean_std                the [mean, std] that Preprocessor.get_f0cwt returns (np.mean / np.std of get_cont_lf0's contour)
  {k}_W                       the transform get_f0cwt was handed by get_lf0_cwt - pycwt is NOT installed, so get_lf0_cwt is replaced by
                              the restated transform (tests/pitch_restate.py cwt_mexican_hat): this array pins nothing about pycwt, it
                              is the input of the two entries below
  {k}_norm, {k}_norm_mean, {k}_norm_std      norm_scale(W)
  {k}_icwt                    inverse_cwt(W[None], scales)
Tracks without two distinct voiced values have no finite transform: their W / norm / icwt entries are left out.
Re-run:  python tests/golden/make_goldens_pitch_features.py
"""
import os
import sys
import warnings

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(OUT))
import pitch_restate as R  # noqa: E402
from oracle import ref_import  # noqa: E402


def main():
    ref_import.install()
    from utils import pitch_tools as PT
    from preprocessor import preprocessor as PP

    scales = R.cwt_scales()
    PP.get_lf0_cwt = lambda x: (R.cwt_mexican_hat(np.squeeze(x)), scales)       # pycwt is absent (see the docstring)
    cfg = {"pitch_norm": "log", "pitch_norm_eps": 1e-9, "use_uv": True}
    arrays = {}
    warnings.simplefilter("ignore")
    for k, f0 in R.FIXTURE_TRACKS.items():
        arrays[f"{k}_f0"] = f0
        uv, c = PT.convert_continuos_f0(f0.copy())
        arrays[f"{k}_ccf0_uv"], arrays[f"{k}_ccf0"] = uv, c
        uv, lf = PT.get_cont_lf0(f0.copy())
        arrays[f"{k}_lf0_uv"], arrays[f"{k}_lf0"] = uv, lf
        y, uv = PT.norm_interp_f0(f0.copy(), cfg)
        arrays[f"{k}_nif0"], arrays[f"{k}_nif0_uv"] = y, uv
        W, _, ms = PP.Preprocessor.get_f0cwt(None, f0.copy())
        arrays[f"{k}_mean_std"] = ms
        if np.isfinite(W).all() and np.isfinite(ms).all() and lf.max() > lf.min():
            arrays[f"{k}_W"] = W
            nrm, m, s = PT.norm_scale(W)
            arrays[f"{k}_norm"], arrays[f"{k}_norm_mean"], arrays[f"{k}_norm_std"] = nrm, m, s
            arrays[f"{k}_icwt"] = PT.inverse_cwt(W[None], scales)
        print(k, len(f0), "mean/std", ms)
    path = os.path.join(OUT, "g19_pitch_chain.npz")
    np.savez_compressed(path, **arrays)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
