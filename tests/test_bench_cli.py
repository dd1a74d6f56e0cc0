"""bench.py's command line and its --dump-outputs writer.  CPU only: runs nothing on a GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (module level: argparse, numpy, scipy only)


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (5, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_levels_dense(tmp_path):
    idx = np.array([0, 3, 6], np.int64)
    lv = np.array([1, 2, 7], np.int32)
    bench.dump_levels(str(tmp_path / "o"), "levels", idx, lv, 7, seed=42)
    got = np.load(tmp_path / "o" / "levels.npy")
    assert got.dtype == np.float32
    assert np.array_equal(got, [1, 0, 0, 2, 0, 0, 7])


def test_dump_levels_sample_is_fixed_and_within_budget(tmp_path):
    n, budget = 1000, 256  # room for 64 float32
    idx = np.arange(0, n, 3, dtype=np.int64)
    lv = (idx % 9 + 1).astype(np.int32)
    dense = np.zeros(n, np.float32)
    dense[idx] = lv
    for d in ("a", "b"):
        bench.dump_levels(str(tmp_path / d), "levels", idx, lv, n, seed=42, budget=budget)
    a, b = np.load(tmp_path / "a" / "levels.npy"), np.load(tmp_path / "b" / "levels.npy")
    assert a.dtype == np.float32 and a.nbytes == budget
    assert np.array_equal(a, b)
    pos = np.sort(np.random.default_rng(42).choice(n, budget // 4, replace=False))
    assert np.array_equal(a, dense[pos])
    assert bench.DUMP_MAX_BYTES <= 64 * 10**6
