"""bench.py --dump-outputs writes float arrays, and past its cap a fixed seeded sample of rows with their row numbers."""
import os

import numpy as np

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_keeps_everything_under_the_cap(tmp_path):
    a = np.arange(3000, dtype=np.float64).reshape(1000, 3) / 7
    f = (np.arange(1000) % 3 == 0).astype(np.uint8)
    bench.dump_outputs(str(tmp_path), {"a": a, "flags": f, "counters": np.array([1.0, 2.0])})
    got = _load(tmp_path)
    assert sorted(got) == ["a", "counters", "flags"]
    assert got["a"].dtype == np.float64 and np.array_equal(got["a"], a)
    assert got["flags"].dtype == np.float32 and np.array_equal(got["flags"], f)


def test_dump_outputs_samples_the_same_rows_past_the_cap(tmp_path, monkeypatch):
    a = np.arange(30000, dtype=np.float64).reshape(10000, 3)
    f = (np.arange(10000) % 5 == 0).astype(np.uint8)
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 64 << 10)
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "flags": f})
    one, two = _load(tmp_path / "one"), _load(tmp_path / "two")
    assert sorted(one) == ["a", "a_rows", "flags", "flags_rows"]
    assert all(np.array_equal(one[k], two[k]) for k in one)
    assert sum(v.nbytes for v in one.values()) <= 64 << 10
    rows = one["a_rows"].astype(np.int64)
    assert len(rows) > 100 and np.all(np.diff(rows) > 0) and np.array_equal(one["a"], a[rows])
    assert np.array_equal(one["flags"], f[one["flags_rows"].astype(np.int64)])
