"""bench.py's options and its output dump, on the CPU: --full and --dump-outputs exist, and dump_outputs() writes
float64 .npy files under the 64 MB limit -- a voxel grid too large for it as the same seeded sample every time."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_DUMP = r"""
import sys
import numpy as np
import bench
n = int(sys.argv[2])
rng = np.random.default_rng(1)
result = dict(T=np.eye(4), pose=np.arange(6.0), hessian=np.ones((6, 6)), iterations=7, n_evaluations=9, converged=True,
              score=-1.5, transform_probability=0.25, nvtl=1.75, n_pairs=123)
leaves = dict(cell=np.arange(n, dtype=np.int64) * 3, count=np.full(n, 6, np.int32), mean=rng.normal(size=(n, 3)),
              cov=rng.normal(size=(n, 3, 3)), icov=rng.normal(size=(n, 3, 3)), center=np.zeros((n, 3), np.float32))
bench.dump_outputs(sys.argv[1], dict(result=result, leaves=leaves))
"""


def _dump(d, n):
    p = subprocess.run([sys.executable, "-c", _DUMP, str(d), str(n)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return {f[:-4]: np.load(os.path.join(str(d), f)) for f in os.listdir(str(d))}


def test_bench_has_full_and_dump_outputs_options():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


def test_dump_outputs_writes_float64_arrays(tmp_path):
    a = _dump(tmp_path, 1000)
    assert set(a) == {"final_transformation", "final_pose", "hessian", "iterations", "n_evaluations", "converged", "score",
                      "transform_probability", "nvtl", "n_pairs", "leaf_cell", "leaf_count", "leaf_mean", "leaf_cov", "leaf_icov"}
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["final_transformation"], np.eye(4)) and a["iterations"].tolist() == [7.0]
    assert a["converged"].tolist() == [1.0] and a["n_pairs"].tolist() == [123.0] and a["score"].tolist() == [-1.5]
    assert np.array_equal(a["leaf_cell"], np.arange(1000) * 3.0) and a["leaf_icov"].shape == (1000, 3, 3)


def test_dump_outputs_samples_a_large_grid_the_same_way_every_time(tmp_path):
    n = 400000   # 184 bytes a leaf: 74 MB whole
    a = _dump(tmp_path / "a", n)
    b = _dump(tmp_path / "b", n)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    m = len(a["leaf_cell"])
    assert 0 < m < n and np.all(np.diff(a["leaf_cell"]) > 0)
    assert a["leaf_mean"].shape == (m, 3) and a["leaf_cov"].shape == (m, 3, 3) and a["leaf_count"].shape == (m,)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
