"""bench.py --dump-outputs: the writer's budget (a fixed, seeded row sample above it) and dtypes, without a GPU."""
import importlib.util
import os

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_every_array_unchanged_under_the_budget(tmp_path):
    bench = _bench()
    arrays = {"embeddings": np.random.default_rng(0).standard_normal((64, 1, 512)).astype(np.float32),
              "match_index": np.arange(64, dtype=np.float64)}
    bench.dump_outputs(str(tmp_path), arrays)
    for name, a in arrays.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == a.dtype and np.array_equal(got, a)


def test_dump_outputs_samples_the_same_rows_above_the_budget(tmp_path):
    bench = _bench()
    arrays = {"embeddings": np.random.default_rng(1).standard_normal((1000, 512)).astype(np.float32),
              "match_score": np.random.default_rng(2).random(1000).astype(np.float32)}
    budget = 256 << 10
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    total = 0
    for name, a in arrays.items():
        got, again = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(got, again)                              # fixed, seeded sample
        assert 0 < got.shape[0] < a.shape[0] and got.shape[1:] == a.shape[1:]
        assert all(any(np.array_equal(r, s) for s in a) for r in got[:5])  # rows of the output, not something else
        total += got.nbytes
    assert total <= budget
