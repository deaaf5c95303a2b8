"""Golden-vector generator for the dataset-preparation kernels - runs ONLY where the reference checkout exists (through
oracle/ref_import.py).

Calls the live reference's own functions unbound (neither uses `self`) and writes tests/golden/g20_preprocess.npz (data only):
  prior_{P}_{M}_{sf}          Preprocessor.beta_binomial_prior_distribution(None, P, M, sf) as float32 [M, P] for the (P, M, sf) of
                              tests/preprocess_restate.py PRIOR_CASES (P = mel frames, M = phonemes: the order of the CALL at :409-413)
  prior_big_rows, prior_big   rows PRIOR_BIG_ROWS of the (1000, 128, 1) prior
  out_{k}_values, out_{k}_kept    the fixture arrays of preprocess_restate.outlier_fixtures() and Preprocessor.remove_outlier(None, v)
  out_order                   the fixture names in the order they were fed to the scaler
  scaler_mean, scaler_scale   sklearn's StandardScaler after partial_fit(kept.reshape(-1, 1)) per array, empty ones skipped as :135-137 does
Every fixture array is checked to keep its values 1e-5 (relative) away from the outlier bounds, so float32 / float64 evaluation agree.
Re-run:  python tests/golden/make_goldens_preprocess.py
"""
import os
import sys
import warnings

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(OUT))
import preprocess_restate as R  # noqa: E402
from oracle import ref_import  # noqa: E402


def main():
    ref_import.install()
    from preprocessor import preprocessor as PP
    from sklearn.preprocessing import StandardScaler

    warnings.simplefilter("ignore")
    arrays = {}
    for P, M, sf in R.PRIOR_CASES:
        a = PP.Preprocessor.beta_binomial_prior_distribution(None, P, M, sf)
        assert a.shape == (M, P)
        arrays[f"prior_{P}_{M}_{sf}"] = a.astype(np.float32)
        print("prior", P, M, sf, "row sums", a.sum(1).min(), a.sum(1).max())
    P, M, sf = R.PRIOR_BIG
    a = PP.Preprocessor.beta_binomial_prior_distribution(None, P, M, sf)
    arrays["prior_big_rows"] = np.array(R.PRIOR_BIG_ROWS)
    arrays["prior_big"] = a[R.PRIOR_BIG_ROWS].astype(np.float32)
    scaler, order = StandardScaler(), []
    for k, v in R.outlier_fixtures().items():
        assert R.bound_margin(v) > 1e-5, (k, R.bound_margin(v))
        kept = PP.Preprocessor.remove_outlier(None, v)
        arrays[f"out_{k}_values"], arrays[f"out_{k}_kept"] = v, kept
        order.append(k)
        if len(kept) > 0:
            scaler.partial_fit(kept.reshape((-1, 1)))
        print("outlier", k, len(v), "->", len(kept))
    arrays["out_order"] = np.array(order)
    arrays["scaler_mean"], arrays["scaler_scale"] = scaler.mean_.copy(), scaler.scale_.copy()
    path = os.path.join(OUT, "g20_preprocess.npz")
    np.savez_compressed(path, **arrays)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
