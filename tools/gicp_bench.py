"""Times of the GICP calls at the C2 workload of bench_configs.py beside the NDT align of the same clouds (tuning aid, not
collected by pytest; no gate):
  - the source and target covariance builds (index build where the cloud has none yet, kNN pass 1, kNN pass 2 -- the tail
    of isolated points, as for fitness --, the covariance kernel), with the kNN kernels separately;
  - one pairing, one evaluation (Hessian and gradient-only) beside a D2D-shaped reference: the ordinary NDT evaluation;
  - one GICP align and one NDT align from the workload's guess.

    python tools/gicp_bench.py               wall times in this process, then the same workload in a child process under
                                             `rocprofv3 --kernel-trace --stats` for the kernel times; writes profiles/gicp.txt
    python tools/gicp_bench.py --workload    the profiled workload itself

Expectations written down before the first run: an evaluation over frozen pairs costs about what a D2D evaluation does, and
pairing dominates an align."""
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 20


def median_ms(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def workload(out):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    cfg = pkg.synth.config_c2()
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=cfg["resolution"], step_size=0.1, trans_epsilon=1e-4,
                                           max_iterations=50)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    out.append("workload %s: %d target points, %d source points" % (cfg["name"], len(cfg["target"]), len(cfg["source"])))

    def rebuild(which):
        pkg.gicpSetParams(ndt, k_neighbours=19)      # drops the cached covariances of both clouds
        pkg.gicpSetParams(ndt, k_neighbours=20)
        pkg.lib().ndt_gicp_export_neighbours(ndt._h, which, None, None, 1 << 62)

    pkg.gicpNeighbours(ndt, "source")
    pkg.gicpNeighbours(ndt, "target")
    for name, which in (("source", pkg.GICP_SOURCE), ("target", pkg.GICP_TARGET)):
        med, lo = median_ms(lambda: rebuild(which))
        _, found = pkg.gicpNeighbours(ndt, name)
        out.append("  covariance build, %-6s (kNN + covariances, index kept)   median %8.3f ms   min %8.3f   (%d points without a covariance)"
                   % (name, med, lo, int((found < 4).sum())))
    T_ndt = ndt.align(cfg["guess"])
    r_ndt = ndt.getResult()
    pose = np.asarray(r_ndt["pose"])
    med, lo = median_ms(lambda: pkg.gicpPair(ndt, pose))
    out.append("  pairing at the NDT result                                   median %8.3f ms   min %8.3f   (%d pairs)" % (med, lo, pkg.gicpPair(ndt, pose)))
    for hess in (True, False):
        med, lo = median_ms(lambda: pkg.evalDerivativesGICP(ndt, pose, compute_hessian=hess, raw=True))
        out.append("  GICP evaluation over the frozen pairs, %-13s        median %8.3f ms   min %8.3f" % ("Hessian" if hess else "gradient only", med, lo))
    med, lo = median_ms(lambda: ndt.evalDerivatives(pose))
    out.append("  NDT evaluation of the same source (point to distribution)   median %8.3f ms   min %8.3f" % (med, lo))
    res = []
    med, lo = median_ms(lambda: res.append(pkg.alignGICP(ndt, cfg["guess"])), reps=5)
    Tg, rg = res[-1]
    info = rg["gicp"]
    out.append("  GICP align from the guess                                   median %8.3f ms   min %8.3f   (%d outer, %d inner iterations, "
               "%d evaluations, %d pairs, converged %d)" % (med, lo, info["outer_iterations"], info["inner_iterations"],
                                                            info["n_evaluations"], info["n_pairs"], rg["converged"]))
    med, lo = median_ms(lambda: ndt.align(cfg["guess"]), reps=5)
    out.append("  NDT align from the guess                                    median %8.3f ms   min %8.3f   (%d iterations)" % (med, lo, r_ndt["iterations"]))
    e_ndt, e_gicp = pkg.synth.pose_error(T_ndt, cfg["gt"]), pkg.synth.pose_error(Tg, cfg["gt"])
    out.append("  distance to the workload's ground truth: NDT %.4f m %.2e rad, GICP %.4f m %.2e rad; GICP to NDT %.4f m %.2e rad"
               % (e_ndt + e_gicp + pkg.synth.pose_error(Tg, T_ndt)))


def kernel_times(out):
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "gicp", "--",
                            sys.executable, os.path.abspath(__file__), "--workload"], capture_output=True, text=True)
        if p.returncode != 0:
            out.append("rocprofv3 exited with %d: %s" % (p.returncode, p.stderr[-500:]))
            return
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    m = re.search(r"k_(gicp|fit)_[a-z_]+(<[^>]*>)?", r["Name"])
                    if m:
                        rows.append((m.group(0), int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
        for lab, calls, avg, lo, hi in sorted(rows):
            out.append("  %-28s calls %5d   avg %9.2f us   min %9.2f   max %9.2f" % (lab, calls, avg, lo, hi))


if __name__ == "__main__":
    lines = []
    if len(sys.argv) > 1 and sys.argv[1] == "--workload":
        workload(lines)
        print("\n".join(lines))
        sys.exit(0)
    lines.append("GICP at C2: wall times of the calls (median of %d, 5 for the aligns), then kernel times of the same workload" % REPS)
    workload(lines)
    lines.append("")
    lines.append("kernel times (rocprofv3 --kernel-trace --stats; both clouds' kernels together -- k_gicp_knn_tail is pass 2, the isolated points)")
    kernel_times(lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(ROOT, "profiles", "gicp.txt"), "w") as f:
        f.write(text)
