"""getFitnessScore cost per call on C2, C3 and C3-wide: index build (the first fitness call after a new target,
minus a query) and query (a fitness call on the cached index), wall clock around the C-ABI call, median of the reps;
next to it the CPU alternative a user would otherwise run: scipy cKDTree build + query (workers=16) in f64.

    python tools/fitness_bench.py [--reps 15] [--out profiles/fitness_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-kdtree", action="store_true")
    a = ap.parse_args()
    pkg = ge.load_package()
    S = pkg.synth
    lines = ["# tools/fitness_bench.py --reps %d  (%s)" % (a.reps, pkg.backend_info()[1])]
    for name, cfg in (("C2", S.config_c2()), ("C3", S.config_c3()), ("C3-wide", S.config_c3_wide())):
        ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=cfg["resolution"])
        ndt.setInputSource(cfg["source"])
        T = cfg["guess"]
        first, query = [], []
        for r in range(a.reps + 2):
            ndt.setInputTarget(cfg["target"])
            ndt.wait()
            t0 = time.perf_counter()
            f = ndt.fitness(T)
            t1 = time.perf_counter()
            ndt.fitness(T)
            t2 = time.perf_counter()
            ndt.fitness(T)
            t3 = time.perf_counter()
            if r >= 2:
                first.append((t1 - t0) * 1e3)
                query.append(min(t2 - t1, t3 - t2) * 1e3)
        q = float(np.median(query))
        b = float(np.median(first)) - q
        ndt.align(T)
        t0 = time.perf_counter()
        ndt.align(T)
        ms_align = (time.perf_counter() - t0) * 1e3
        ln = ("%-8s target %7d source %6d | index build %.3f ms  query %.3f ms  (build+query %.3f ms; one align %.3f ms)"
              " | fitness %.6g over %d / %d" % (name, len(cfg["target"]), len(cfg["source"]), b, q, b + q, ms_align,
                                              f["fitness_score"], f["n_inliers"], f["n_points"]))
        if not a.no_kdtree:
            from scipy.spatial import cKDTree
            qs = ndt.transformSource(T).astype(np.float64)
            t0 = time.perf_counter()
            tree = cKDTree(np.asarray(cfg["target"], np.float64))
            t1 = time.perf_counter()
            d, _ = tree.query(qs, workers=16)
            t2 = time.perf_counter()
            ln += " | cKDTree build %.1f ms query %.1f ms (fitness %.6g)" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3,
                                                                              float(np.mean(d * d)))
        print(ln, flush=True)
        lines.append(ln)
        ndt.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
