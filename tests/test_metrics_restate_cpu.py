"""CPU: the float64 restatement of the objective-evaluation kernels (tests/metrics_restate.py, the yardstick of
tests/test_metrics_gpu.py) against closed forms, brute force and hand-worked numbers; `ctts_amd.metrics` has no CPU path."""
import numpy as np
import pytest
import torch

from ctts_amd import metrics as M
from ctts_amd._lib import CttsError
from tests import metrics_restate as R


# ------------------------------------------------------------------------------------------------------------------------ cepstrum
@pytest.mark.parametrize("M_", [20, 80])
def test_dct_of_a_constant_mel_is_zero(M_):
    c = R.mel_cepstrum(np.full((M_, 3), -4.25), 13)
    assert c.shape == (3, 13)
    assert np.abs(c).max() < 1e-12


@pytest.mark.parametrize("M_,q", [(80, 1), (80, 5), (80, 13), (20, 7)])
def test_dct_of_a_basis_cosine_has_one_coefficient(M_, q):
    m = np.arange(M_)
    mel = np.cos(np.pi * q * (m + 0.5) / M_)[:, None]
    c = R.mel_cepstrum(mel, 13)[0]
    want = np.zeros(13)
    want[q - 1] = np.sqrt(M_ / 2.0)
    assert np.abs(c - want).max() < 1e-12


def test_dct_rows_are_orthonormal():
    D = R.dct_matrix(80, 32)
    assert np.abs(D @ D.T - np.eye(32)).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------------ DP
@pytest.mark.parametrize("Lx,Ly", [(a, b) for a in range(1, 6) for b in range(1, 6)])
def test_dp_optimum_equals_brute_force(Lx, Ly):
    rng = np.random.default_rng(100 * Lx + Ly)
    for _ in range(4):
        d = rng.uniform(0.1, 2.0, (Lx, Ly))
        A, dirs = R.accumulate(d)
        want = R.brute_force_cost(d)
        assert A[-1, -1] == pytest.approx(want, rel=1e-13)
        path = R.backtrack(dirs)
        assert R.is_monotone_path(path, Lx, Ly)
        assert R.path_cost(d, path) == pytest.approx(want, rel=1e-13)
        assert np.array_equal(R.accumulate_fast(d), A)


def test_path_count_is_the_delannoy_number():
    assert [len(R.monotone_paths(n, n)) for n in (1, 2, 3, 4)] == [1, 3, 13, 63]


def test_tie_rule_prefers_diagonal_then_up_then_left():
    # all costs equal: every predecessor ties wherever two exist, the diagonal must win, so a square gives the pure diagonal
    _, dirs = R.accumulate(np.ones((4, 4)))
    assert R.backtrack(dirs) == [(i, i) for i in range(4)]
    # (1,1) with A(0,0) = 5 and A(0,1) = A(1,0) = 1: up and left tie below the diagonal, up = (i-1, j) wins
    d = np.array([[5.0, -4.0], [-4.0, 1.0]])
    A, dirs = R.accumulate(d)
    assert A[0, 1] == A[1, 0] == 1.0 and dirs[1, 1] == 1
    assert R.backtrack(dirs) == [(0, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("L", [1, 2, 65])
def test_identical_sequences_give_zero_cost_and_the_diagonal(L):
    x = np.random.default_rng(L).standard_normal((L, 13))
    cost, path = R.dtw(x, x.copy())
    assert cost == 0.0
    assert path == [(i, i) for i in range(L)]


@pytest.mark.parametrize("L", [1, 3, 65])
def test_repeated_frames_give_zero_cost_and_the_staircase(L):
    x = np.random.default_rng(7 + L).standard_normal((L, 13))
    y = np.repeat(x, 2, axis=0)
    cost, path = R.dtw(x, y)
    assert cost == 0.0
    assert len(path) == 2 * L
    assert path == [(i, 2 * i + s) for i in range(L) for s in (0, 1)]


def test_empty_sequence():
    assert R.dtw(np.zeros((0, 13)), np.zeros((5, 13))) == (0.0, [])


# ------------------------------------------------------------------------------------------------------------------------ path sums
def test_path_metrics_by_hand():
    f0_x = [100.0, 0.0, 200.0, 200.0]
    f0_y = [200.0, 0.0, 100.0, 0.0, 400.0]
    path = [(0, 0), (1, 1), (1, 2), (2, 2), (2, 3), (3, 4)]
    # (0,0): 100 / 200 -> -1200 cents; (1,1): both unvoiced; (1,2): differs; (2,2): 200 / 100 -> +1200; (2,3): differs; (3,4): 200 / 400 -> -1200
    pairs, both, sq, differ = R.path_metrics(path, f0_x, f0_y)
    assert (pairs, both, differ) == (6, 3, 2)
    assert sq == pytest.approx(3 * 1200.0 ** 2, rel=1e-15)
    assert np.sqrt(sq / both) == pytest.approx(1200.0)
    assert R.path_metrics([], f0_x, f0_y) == (0, 0, 0.0, 0)


def test_mcd_constant():
    assert R.MCD_DB == pytest.approx(6.141851463713754, rel=1e-14)
    assert M.MCD_DB == R.MCD_DB


# ------------------------------------------------------------------------------------------------------------------------ no CPU path
def test_metrics_refuse_host_tensors():
    mel, f0 = torch.zeros(1, 80, 6), torch.zeros(1, 6)
    x = torch.zeros(1, 6, 13)
    lens = torch.tensor([6], dtype=torch.int32)
    path = torch.zeros(1, 11, 2, dtype=torch.int32)
    with pytest.raises(CttsError):
        M.mel_cepstrum(mel, lens)
    with pytest.raises(CttsError):
        M.dtw(x, lens, x, lens)
    with pytest.raises(CttsError):
        M.path_metrics(path, lens, f0, f0)
    with pytest.raises(CttsError):
        M.compare_mels(mel, lens, mel, lens, f0, f0)
    with pytest.raises(CttsError):
        M.compare_wavs(torch.zeros(1, 4096), None, torch.zeros(1, 4096), None, None)
