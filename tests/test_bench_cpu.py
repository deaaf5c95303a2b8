"""CPU: bench.py's command line (a plain run measures the headline only; the extra measurements sit behind --full) and its
--dump-outputs writer (float arrays, a fixed seeded sample of long vectors, at most 64 MB per run)."""
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_command_line_is_lean(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.no_cpu_baseline and a.dump_outputs == "out"


def _fake_step(n_params, seed):
    g = torch.Generator().manual_seed(seed)
    params = []
    for n in n_params:
        p = torch.randn(n, generator=g)
        p.grad = torch.randn(n, generator=g)
        params.append(p)
    terms = (torch.tensor(3.5), torch.tensor(1.25), {"a": torch.tensor(0.5), "b": torch.tensor(0.25)}, None, torch.zeros(1))
    return SimpleNamespace(params=params, loss_terms=terms)


def test_dump_outputs_small_vectors_whole(tmp_path):
    bench = _bench()
    step = _fake_step([30, 7, 13], 0)
    names = bench.dump_outputs(step, str(tmp_path / "d"))
    assert names == ["grads", "loss_terms", "params"]
    out = {n: np.load(tmp_path / "d" / (n + ".npy")) for n in names}
    assert out["loss_terms"].dtype == np.float64 and out["params"].dtype == out["grads"].dtype == np.float32
    lt = out["loss_terms"]
    assert lt.shape == (6,) and list(lt[[0, 1, 2, 3, 5]]) == [3.5, 1.25, 0.5, 0.25, 0.0] and np.isnan(lt[4])
    assert np.array_equal(out["params"], torch.cat(step.params).numpy())
    assert np.array_equal(out["grads"], torch.cat([p.grad for p in step.params]).numpy())


def test_dump_outputs_samples_long_vectors_at_fixed_positions(tmp_path):
    bench = _bench()
    step = _fake_step([4000, 1000], 1)
    bench.dump_outputs(step, str(tmp_path / "a"), sample=512)
    bench.dump_outputs(step, str(tmp_path / "b"), sample=512)
    full_p, full_g = torch.cat(step.params).numpy(), torch.cat([p.grad for p in step.params]).numpy()
    for name, full in (("params", full_p), ("grads", full_g)):
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.shape == (512,) and np.array_equal(x, y)
        assert np.isin(x, full).all()
    # the same positions in both vectors
    pos = [int(np.flatnonzero(full_p == v)[0]) for v in np.load(tmp_path / "a" / "params.npy")]
    assert np.array_equal(np.load(tmp_path / "a" / "grads.npy"), full_g[pos])
    # the default sample keeps a real run's dump within 64 MB
    assert 2 * 4 * bench.DUMP_SAMPLE + 8 * 64 < 64 * 2 ** 20
