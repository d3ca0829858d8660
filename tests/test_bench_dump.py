"""CPU: bench.py --dump-outputs writes what the timed path's last step returned; above its byte budget, a fixed seeded sample of whole
output frames with their indices (the files stay inside the budget, and the same output gives the same files)."""
import os

import numpy as np

import bench


def _files(d):
    return {n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_bench_dump_within_budget_is_the_whole_output(tmp_path):
    y = np.random.default_rng(1).standard_normal((1000, 8)).astype(np.float32)
    bench.dump_outputs(str(tmp_path), "output", 917, 1000, y, 1 << 20)
    f = _files(tmp_path)
    assert sorted(f) == ["output.npy", "output_counts.npy"]
    assert f["output.npy"].dtype == np.float32 and np.array_equal(f["output.npy"], y)
    assert f["output_counts.npy"].dtype == np.float64 and list(f["output_counts.npy"]) == [917, 1000]


def test_bench_dump_over_budget_is_a_fixed_sample_of_whole_frames(tmp_path):
    y = np.random.default_rng(2).standard_normal((100000, 8)).astype(np.float32)        # 3.2 MB
    budget = 1 << 20
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "output_rank1", 91875, 100000, y, budget)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert sorted(a) == ["output_rank1.npy", "output_rank1_counts.npy", "output_rank1_rows.npy"]
    assert all(np.array_equal(a[n], b[n]) for n in a)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in a) <= budget
    rows = a["output_rank1_rows.npy"]
    assert rows.dtype == np.float64 and len(rows) > 20000 and np.all(np.diff(rows) > 0) and 0 <= rows[0] and rows[-1] < len(y)
    assert a["output_rank1.npy"].dtype == np.float32 and np.array_equal(a["output_rank1.npy"], y[rows.astype(np.int64)])
