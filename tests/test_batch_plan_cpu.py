"""CPU: invariants of the length-balanced tile order of the batched, length-limited GEMM launches (csrc/batch_plan.h, the header the
device code compiles), checked by a small C++ program built with g++: every (batch, tile) item in exactly one slot, active items in the
first slots and the rest after them in plain order, active work non-increasing in rank (ties by batch, then tile), two builds equal;
and the per-CU loads the order was made for, on the canonical fs2 batch and on uniform lengths."""
import os
import random
import subprocess

import pytest

from ctts_amd.synthetic import CANONICAL_SRC_LENS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the two launch geometries of the fs2 attention (2 heads x 128): M N K of a batch as functions of T, lim_m lim_n lim_k, write_all
S_TYPE = (lambda T: (T, T, 128), (1, 1, 0), 0)        # S = Q K^T, dP = dO V^T
MAP_PRODUCT = (lambda T: (T, 128, T), (1, 0, 1), 1)   # O = P V, dV, dQ, dK


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bp") / "batch_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "native", "batch_plan_check.cpp"), "-o", exe], check=True)
    return exe


def check(checker, geom, T, lens, nbins, nb1=2, tile=(64, 64, 32)):
    dims, lim, write_all = geom
    argv = [*dims(T), *tile, nb1, *lim, write_all, nbins, *lens]
    r = subprocess.run([checker] + [str(v) for v in argv], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (argv, r.stdout, r.stderr)
    n_active, n_listed, mx, mn, total = (int(v) for v in r.stdout.split()[1:])
    return n_active, n_listed, mx, mn, total


def _random_lens(T, seed):
    rng = random.Random(seed)
    lens = [0, 1, 64, 65, T] + [rng.randint(0, T) for _ in range(rng.randint(0, 11))]
    rng.shuffle(lens)
    return lens


@pytest.mark.parametrize("geom", [S_TYPE, MAP_PRODUCT], ids=["s_type", "map_product"])
@pytest.mark.parametrize("T,nbins,seed", [(192, 256, 0), (200, 8, 1), (1024, 256, 2), (130, 5, 3), (65, 1, 4), (700, 256, 5)])
def test_plan_invariants(checker, geom, T, nbins, seed):
    lens = _random_lens(T, seed)
    n_active, n_listed, _, _, _ = check(checker, geom, T, lens, nbins)
    tm = lambda L: -(-L // 64)
    want = sum(2 * tm(L) * (tm(L) if geom is S_TYPE else 2) for L in lens)
    assert n_active == want
    assert n_listed == (n_active if geom is S_TYPE else 2 * len(lens) * tm(T) * 2)


def test_all_empty_and_all_full(checker):
    for geom in (S_TYPE, MAP_PRODUCT):
        assert check(checker, geom, 192, [0, 0, 0], 256)[0] == 0
        n_active, n_listed, mx, mn, _ = check(checker, geom, 192, [192] * 4, 4)
        assert n_active == n_listed and mx == mn


def test_per_cu_load_of_the_canonical_batch(checker):
    """O = P V at the decoder size (16 utterances x 2 heads, T = 1024, 64 x 64 x 32 tiles) over 256 CUs, in K-blocks: plain order
    gives the most loaded CU 102 of a mean of 76.1; uniform lengths balance exactly."""
    n_active, _, mx, mn, total = check(checker, MAP_PRODUCT, 1024, [8 * s for s in CANONICAL_SRC_LENS], 256)
    assert n_active == 776 and abs(total / 256 - 76.1) < 0.05
    assert mx <= 88 and mn >= 72
    for L, mean in ((768, 72), (512, 32)):
        _, _, mx, mn, total = check(checker, MAP_PRODUCT, 1024, [L] * 16, 256)
        assert mx == mean and mn == mean and total == 256 * mean
