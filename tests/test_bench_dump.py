"""bench.py --dump-outputs: the writer alone (no GPU)."""
import importlib.util
import os
import sys
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module(monkeypatch):
    """bench.py as a module, without leaving its import-time changes (environment, sys.path) in this process"""
    monkeypatch.setattr(sys, "path", list(sys.path))
    spec = importlib.util.spec_from_file_location("bench_for_dump", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    with mock.patch.dict(os.environ):
        spec.loader.exec_module(bench)
    return bench


def test_dump_below_the_limit_writes_every_item(tmp_path, monkeypatch):
    bench = _bench_module(monkeypatch)
    rows = np.arange(10 * 48).reshape(10, 48) % 256
    bench.dump_outputs(str(tmp_path), {"commitments": rows, "status": np.zeros(10, dtype=np.int32)})
    assert sorted(os.listdir(tmp_path)) == ["commitments.npy", "status.npy"]
    got = np.load(tmp_path / "commitments.npy")
    assert got.dtype == np.float32 and np.array_equal(got, rows)


def test_dump_above_the_limit_keeps_a_seeded_sample(tmp_path, monkeypatch):
    """above the size limit every array keeps a sample of its items, fixed by the seed: the same from run to run"""
    bench = _bench_module(monkeypatch)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10000)
    rows = np.arange(1000 * 48, dtype=np.float64).reshape(1000, 48) % 256
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"commitments": rows, "status": np.arange(1000) % 3})
    got = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["commitments.npy", "commitments_sample_index.npy", "status.npy", "status_sample_index.npy"]
    assert sum(a.nbytes for a in got.values()) <= 10000
    idx = got["commitments_sample_index.npy"].astype(np.int64)
    assert 0 < len(idx) < 1000 and np.array_equal(got["commitments.npy"], rows[idx].astype(np.float32))
    assert np.array_equal(got["status_sample_index.npy"], got["commitments_sample_index.npy"])  # equal lengths: the same items
    assert np.array_equal(got["status.npy"], (idx % 3).astype(np.float32))
    for f, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f))
