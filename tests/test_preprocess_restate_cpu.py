"""CPU: the float64 restatements of tests/preprocess_restate.py (the yardstick of tests/test_preprocess_gpu.py) against the live
reference's own results (tests/golden/g20_preprocess.npz: scipy's betabinom through `beta_binomial_prior_distribution`, numpy's
percentile through `remove_outlier`, sklearn's StandardScaler.partial_fit), the host-side Chan merge, and the `attn_prior` option of the
host data path.

Prior bar: relative <= 1e-6 wherever the golden is >= 1e-30, absolute <= 1e-37 below.  The float64 closed form rounded to float32 lies
within 6e-8 of scipy at every shape stored (one float32 rounding), which leaves more than 10x for lgamma error; an absolute-only bar
would test nothing, because 39 % of a 1024 x 128 prior is below 1e-20."""
import numpy as np
import pytest

from ctts_amd import data as D
from ctts_amd.preprocess import merge_moments
from tests import preprocess_restate as R
from tests.preprocess_restate import assert_prior_close
from tests.util import load_golden, synthetic_samples


@pytest.fixture(scope="module")
def g():
    return load_golden("g20_preprocess")


@pytest.mark.parametrize("P,M,sf", R.PRIOR_CASES)
def test_prior_restatement_matches_reference(g, P, M, sf):
    want = g[f"prior_{P}_{M}_{sf}"]
    assert want.shape == (M, P)                               # rows = phonemes, columns = mel frames
    assert_prior_close(R.attention_prior(M, P, sf).astype(np.float32), want, f"prior {P}x{M} sf {sf}")


def test_prior_restatement_matches_reference_rows_of_1000x128(g):
    P, M, sf = R.PRIOR_BIG
    rows = list(g["prior_big_rows"])
    assert rows == R.PRIOR_BIG_ROWS
    assert_prior_close(R.attention_prior(M, P, sf)[rows].astype(np.float32), g["prior_big"], "prior 1000x128 rows")


def test_prior_keeps_the_reference_quirk(g):
    """n is the MEL length and t = n is never emitted: rows do not sum to 1"""
    sums = R.attention_prior(55, 440).sum(1)
    assert sums.min() < 0.9 and sums.max() <= 1.0 + 1e-9
    assert R.attention_prior(1, 1)[0, 0] == pytest.approx(0.5, rel=1e-12)


def test_outlier_kept_sets_match_reference(g):
    fx = R.outlier_fixtures()
    assert list(g["out_order"]) == list(fx)
    assert sorted(len(v) for k, v in fx.items() if k.startswith("n")) == [1, 2, 3, 4, 5, 101, 870]
    for k, v in fx.items():
        assert np.array_equal(g[f"out_{k}_values"], v), k
        assert R.bound_margin(v) > 1e-5, k
        assert np.array_equal(v[R.outlier_keep(v)], g[f"out_{k}_kept"]), k
    assert R.outlier_keep(fx["const"]).sum() == 0 and R.outlier_keep(fx["n1"]).sum() == 0


def test_mean_std_match_partial_fit(g):
    fx = R.outlier_fixtures()
    mean, std = R.dataset_mean_std(fx.values())
    assert abs(mean - g["scaler_mean"][0]) <= 1e-9 * abs(g["scaler_mean"][0])
    assert abs(std - g["scaler_scale"][0]) <= 1e-9 * abs(g["scaler_scale"][0])
    trip = [R.moments(v) for v in fx.values()]                # the Chan merge of the package, fed the restated triples in order
    n, m, s = merge_moments([t[0] for t in trip], [t[1] for t in trip], [t[2] for t in trip])
    assert n == sum(len(g[f"out_{k}_kept"]) for k in fx)
    assert abs(m - g["scaler_mean"][0]) <= 1e-9 * abs(g["scaler_mean"][0])
    assert abs(s - g["scaler_scale"][0]) <= 1e-9 * abs(g["scaler_scale"][0])


def test_trim_restatement_on_hand_made_signals():
    """no librosa here: the restatement is checked against what its definition says on signals whose answer is known"""
    hop = 256
    x = np.zeros(4000)
    assert R.trim_silence(x, 23) == (0, 4000)                # digital silence: every frame is 0 dB below the reference (as in librosa)
    x = 0.5 * np.sin(np.arange(4000) * 0.3)
    assert R.trim_silence(x, 60) == (0, 4000)
    x = np.zeros(22050)
    x[5000:15000] = 0.5 * np.sin(np.arange(10000) * 0.3)
    s, e = R.trim_silence(x, 23)
    assert s % hop == 0 and 5000 - 1024 < s <= 5000 and 15000 <= e < 15000 + 1024 and (e % hop == 0 or e == len(x))
    with pytest.raises(ValueError):
        R.trim_silence(np.zeros(512), 23)


# ---- the attn_prior option of the host data path ---------------------------------------------------------------------------------
def test_collate_files_is_unchanged_and_device_needs_no_field():
    samples = synthetic_samples(10, 6, True)
    ref = D.collate(samples, 4, sort=True, learn_alignment=True)
    files = D.collate(samples, 4, sort=True, learn_alignment=True, attn_prior="files")
    stripped = [{k: v for k, v in s.items() if k != "attn_prior"} for s in samples]
    dev = D.collate(stripped, 4, sort=True, learn_alignment=True, attn_prior="device")
    assert len(ref) == len(files) == len(dev) == 3
    for a, b, c in zip(ref, files, dev):
        assert len(a) == len(b) == len(c) == 20
        for i, (x, y, z) in enumerate(zip(a, b, c)):
            if isinstance(x, np.ndarray):
                assert np.array_equal(x, y) and x.dtype == y.dtype, i
            else:
                assert x == y or (x is None and y is None), i
            if i == 18:
                assert x is not None and z is None
            elif isinstance(x, np.ndarray):
                assert np.array_equal(x, z) and x.dtype == z.dtype, i
            else:
                assert x == z or (x is None and z is None), i
    with pytest.raises(KeyError):
        D.collate(stripped, 4, learn_alignment=True)                                     # "files" still needs the field
    with pytest.raises(ValueError):
        D.collate(samples, 4, learn_alignment=True, attn_prior="host")


def test_pack_reserves_a_device_only_prior_segment():
    samples = synthetic_samples(6, 7, True)
    b_files = D.collate(samples, 6, learn_alignment=True)[0]
    b_dev = D.collate(samples, 6, learn_alignment=True, attn_prior="device")[0]
    pf, pd = D.PackedBatch.pack(b_files, pin=False), D.PackedBatch.pack(b_dev, pin=False, attn_prior="device", scaling_factor=0.5)
    assert "attn_priors" in pf.layout and not pf.device_layout and pf.device_bytes == pf.host.numel()
    assert "attn_priors" not in pd.layout and pd.host_views()[12] is None
    o, shape, dt = pd.device_layout["attn_priors"]
    assert shape == tuple(b_files[18].shape) and o % 256 == 0 and o >= pd.host.numel() - 255
    assert pd.device_bytes == o + 4 * int(np.prod(shape)) and pd.prior_scaling_factor == 0.5
    for k, v in pd.layout.items():                          # every uploaded field sits where the "files" batch has it
        assert pf.layout[k] == v, k
    with pytest.raises(ValueError):
        D.PackedBatch.pack(b_files, pin=False, attn_prior="device")
