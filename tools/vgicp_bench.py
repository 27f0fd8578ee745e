"""Times of the voxelised-GICP calls at the C2 workload of bench_configs.py beside the GICP align and the NDT align of the same
clouds from the same guess in the same process (tuning aid, not collected by pytest; no gate):
  - the voxel table's build alone (both clouds' covariances cached), and from cold with the target's covariances;
  - one evaluation, Hessian and gradient only, as a call;
  - ndt_align_vgicp under DIRECT1 and DIRECT7 with everything cached, for a new scan (the source's covariances from cold, the
    table cached) and with everything cold;
  - ndt_align_gicp and ndt_align beside them.

    python tools/vgicp_bench.py               wall times in this process, then the same workload in a child process under
                                              `rocprofv3 --kernel-trace --stats` for the kernel times; writes profiles/vgicp.txt
    python tools/vgicp_bench.py --workload    the profiled workload itself

Expectation written down before the first run, not a gate: the align proper costs about what a D2D align does (one
evaluation is the D2D kernel's arithmetic with up to seven partners), and per scan the source's kNN (7.2 ms in
profiles/gicp.txt) then dominates."""
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


def timed_ms(fn, reps=REPS, before=None):
    """median and minimum of fn()'s wall time; before() runs untimed in front of every repetition"""
    ts = []
    for _ in range(reps):
        if before:
            before()
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
    out.append("workload %s: %d target points, %d source points, resolution %.2f" % (cfg["name"], len(cfg["target"]), len(cfg["source"]),
                                                                                 cfg["resolution"]))
    L = pkg.lib()

    def drop_all():
        pkg.gicpSetParams(ndt, k_neighbours=19)      # drops the cached covariances of both clouds and the table
        pkg.gicpSetParams(ndt, k_neighbours=20)

    def covariances(which):
        L.ndt_gicp_export_neighbours(ndt._h, which, None, None, 1 << 62)

    def drop_table_only():
        drop_all()
        covariances(pkg.GICP_SOURCE)
        covariances(pkg.GICP_TARGET)

    info = pkg.vgicpInfo(ndt)
    out.append("  table: %d voxels of %d leaves hold %d of the %d target points; without a covariance: %d target, %d source points"
               % (info["n_voxels"], info["n_leaves"], info["n_target_points_in_voxels"], len(cfg["target"]),
                  info["n_target_without_covariance"], info["n_source_without_covariance"]))
    med, lo = timed_ms(lambda: pkg.vgicpInfo(ndt), before=drop_table_only)
    out.append("  table build alone (keys, sort, per-leaf sums, counts read back)     median %8.3f ms   min %8.3f" % (med, lo))
    med, lo = timed_ms(lambda: covariances(pkg.GICP_TARGET), before=drop_all)
    out.append("  target covariances alone (kNN + covariances, index kept)            median %8.3f ms   min %8.3f" % (med, lo))
    T_ndt = ndt.align(cfg["guess"])
    r_ndt = ndt.getResult()
    pose = np.asarray(r_ndt["pose"])
    results = {}
    for name, method in (("DIRECT1", pkg.DIRECT1), ("DIRECT7", pkg.DIRECT7)):
        ndt.setNeighborhoodSearchMethod(method)
        for hess in (True, False):
            med, lo = timed_ms(lambda: pkg.evalDerivativesVGICP(ndt, pose, compute_hessian=hess, raw=True))
            out.append("  %s evaluation at the NDT result, %-13s                   median %8.3f ms   min %8.3f"
                       % (name, "Hessian" if hess else "gradient only", med, lo))
        res = []
        med, lo = timed_ms(lambda: res.append(pkg.alignVGICP(ndt, cfg["guess"])), reps=5)
        Tv, rv = res[-1]
        vi = rv["vgicp"]
        out.append("  %s VGICP align from the guess, everything cached                  median %8.3f ms   min %8.3f   (%d iterations, %d "
                   "evaluations, %d pairs of %d points, converged %d)"
                   % (name, med, lo, rv["iterations"], rv["n_evaluations"], vi["n_pairs"], vi["n_source_with_pairs"], rv["converged"]))
        med, lo = timed_ms(lambda: pkg.alignVGICP(ndt, cfg["guess"]), reps=5, before=lambda: ndt.setInputSource(cfg["source"]))
        out.append("  %s VGICP align of a new scan (source covariances from cold)       median %8.3f ms   min %8.3f" % (name, med, lo))
        med, lo = timed_ms(lambda: pkg.alignVGICP(ndt, cfg["guess"]), reps=5, before=drop_all)
        out.append("  %s VGICP align, both clouds' covariances and the table from cold  median %8.3f ms   min %8.3f" % (name, med, lo))
        results[name] = Tv
    ndt.setNeighborhoodSearchMethod(pkg.DIRECT7)
    res = []
    med, lo = timed_ms(lambda: res.append(pkg.alignGICP(ndt, cfg["guess"])), reps=5)
    Tg, rg = res[-1]
    out.append("  GICP align from the guess, covariances cached                           median %8.3f ms   min %8.3f   (%d outer, %d inner "
               "iterations, %d evaluations, %d pairs, converged %d)" % (med, lo, rg["gicp"]["outer_iterations"], rg["gicp"]["inner_iterations"],
                                                                        rg["gicp"]["n_evaluations"], rg["gicp"]["n_pairs"], rg["converged"]))
    med, lo = timed_ms(lambda: ndt.align(cfg["guess"]), reps=5)
    out.append("  NDT align from the guess (DIRECT7)                                      median %8.3f ms   min %8.3f   (%d iterations)"
               % (med, lo, r_ndt["iterations"]))
    err = pkg.synth.pose_error
    out.append("  distance to the workload's ground truth: NDT %.4f m %.2e rad, GICP %.4f m %.2e rad, VGICP DIRECT1 %.4f m %.2e rad, "
               "VGICP DIRECT7 %.4f m %.2e rad" % (err(T_ndt, cfg["gt"]) + err(Tg, cfg["gt"]) + err(results["DIRECT1"], cfg["gt"])
                                                   + err(results["DIRECT7"], cfg["gt"])))
    out.append("  VGICP to GICP: DIRECT1 %.4f m %.2e rad, DIRECT7 %.4f m %.2e rad" % (err(results["DIRECT1"], Tg) + err(results["DIRECT7"], Tg)))


def kernel_times(out):
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "vgicp", "--",
                            sys.executable, os.path.abspath(__file__), "--workload"], capture_output=True, text=True)
        if p.returncode != 0:
            out.append("rocprofv3 exited with %d: %s" % (p.returncode, p.stderr[-500:]))
            return
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    m = re.search(r"k_(vgicp|gicp|eval_rows)_[a-z_]+(<[^>]*>)?", r["Name"])
                    if m:
                        rows.append((m.group(0), int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
        for lab, calls, avg, lo, hi in sorted(rows):
            out.append("  %-34s calls %5d   avg %9.2f us   min %9.2f   max %9.2f" % (lab, calls, avg, lo, hi))


if __name__ == "__main__":
    lines = []
    if len(sys.argv) > 1 and sys.argv[1] == "--workload":
        workload(lines)
        print("\n".join(lines))
        sys.exit(0)
    lines.append("VGICP at C2 on one MI355X: wall times of the calls (median of %d, 5 for the aligns), then kernel times of the same workload" % REPS)
    workload(lines)
    lines.append("")
    lines.append("kernel times (rocprofv3 --kernel-trace --stats; k_vgicp_eval<Hessian, DIRECT7>; the table's sort kernels are k_sort_* of ndt_sort.hip, "
                 "not listed)")
    kernel_times(lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(ROOT, "profiles", "vgicp.txt"), "w") as f:
        f.write(text)
