"""bench.py --dump-outputs on the CPU: float64 files of what the timed step returned, the size
bound, and the seeded sample of rows that keeps two runs comparable element for element."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402


def test_dump_outputs_writes_every_array_as_float64(tmp_path):
    m = np.arange(24.0).reshape(4, 2, 3)
    rec = bench.dump_outputs(str(tmp_path), {"moments": m, "status": np.array([0, 1, 0, 2], np.int32)})
    assert not rec["sampled"] and rec["files"] == {"moments": [4, 2, 3], "status": [4]}
    got, st = np.load(tmp_path / "moments.npy"), np.load(tmp_path / "status.npy")
    assert got.dtype == np.float64 and np.array_equal(got, m)
    assert st.dtype == np.float64 and st.tolist() == [0, 1, 0, 2]


def test_dump_outputs_keeps_the_same_rows_of_every_array_under_the_bound(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 200_000)
    n = 10_000
    m = np.arange(n * 12, dtype=np.float64).reshape(n, 2, 6)
    st = (np.arange(n) % 3).astype(np.int32)
    for d in ("a", "b"):
        rec = bench.dump_outputs(str(tmp_path / d), {"moments": m, "status": st})
        assert rec["sampled"]
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= 200_000
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    assert np.array_equal(rows, np.load(tmp_path / "b" / "sample_rows.npy"))
    idx = rows.astype(np.int64)
    assert len(idx) > n // 10 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "moments.npy"), m[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "status.npy"), st[idx])
