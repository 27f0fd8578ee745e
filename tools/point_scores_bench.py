"""Kernel times of the per-point scoring calls on C2 and C3 at the aligned pose (tuning aid, not collected by pytest):
k_point_scores, the filter's three compaction kernels, and the score-only launch behind ndt_score_transform on the same
handle -- the launch whose pair work k_point_scores repeats, plus 28 bytes of stores per point.

    python tools/point_scores_bench.py            both configs, each in a child process under
                                                  `rocprofv3 --kernel-trace --stats`; writes profiles/point_scores.txt
    python tools/point_scores_bench.py --workload c2|c3    the profiled workload itself

Expectation written down before the first run: k_point_scores costs about what the score-only k_derivatives launch costs."""
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 200
METHODS = ("DIRECT7", "DIRECT1", "KDTREE", "DIRECT26")


def workload(name):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    cfg = {"c2": pkg.synth.config_c2, "c3": pkg.synth.config_c3}[name]()
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=cfg["resolution"], step_size=0.1, trans_epsilon=1e-4,
                                           max_iterations=50)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    T = ndt.align(cfg["guess"])
    nvs = ndt.scorePoints(T)["nearest_voxel_score"]
    pos = sorted(nvs[nvs > 0])
    thr = float(pos[len(pos) // 2])
    for m in METHODS:
        ndt.setParams(search_method=getattr(pkg, m))
        for _ in range(REPS):
            ndt.scoreTransform(T)
            ndt.scorePoints(T)   # all four outputs: 28 bytes of stores per point
    ndt.setParams(search_method=pkg.DIRECT7)
    for _ in range(REPS):
        ndt.filterSource(T, thr)
    print("workload %s: %d source points, threshold %.6f keeps %d" % (name, len(nvs), thr, int((nvs >= thr).sum())))


NB_NAMES = {"0": "DIRECT1", "1": "DIRECT7", "2": "KDTREE", "3": "DIRECT26", "4": "union", "5": "DIRECT1 packed", "6": "DIRECT7 packed"}


def label(kernel):
    m = re.search(r"k_point_scores<(\d)>", kernel)
    if m:
        return "k_point_scores            %-9s" % NB_NAMES[m.group(1)]
    m = re.search(r"k_derivatives<(\w+), 3, (\d), (\w+)>", kernel)
    if m:
        return "k_derivatives score-only  %-9s" % NB_NAMES[m.group(2)]
    m = re.search(r"k_filter_[a-z]+", kernel)
    return m.group(0) if m else None


def profile(name, out):
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ps", "--",
                            sys.executable, os.path.abspath(__file__), "--workload", name], capture_output=True, text=True)
        said = [ln for ln in p.stdout.splitlines() if ln.startswith("workload ")]
        out.append(said[-1] if said else "(no workload output)")
        if p.returncode != 0:
            out.append("rocprofv3 exited with %d: %s" % (p.returncode, p.stderr[-500:]))
            return
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    lab = label(r["Name"])
                    if lab and int(r["Calls"]) >= REPS:
                        rows.append((lab, int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3,
                                     float(r["MaxNs"]) / 1e3))
        for lab, calls, avg, lo, hi in sorted(rows):
            out.append("  %-40s calls %5d   avg %8.2f us   min %8.2f   max %8.2f" % (lab, calls, avg, lo, hi))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--workload":
        workload(sys.argv[2])
        sys.exit(0)
    lines = ["per-point scores: kernel times at the aligned pose (rocprofv3 --kernel-trace --stats, %d calls each)" % REPS]
    for cfg in ("c2", "c3"):
        lines.append("")
        lines.append("== %s ==" % cfg.upper())
        profile(cfg, lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(ROOT, "profiles", "point_scores.txt"), "w") as f:
        f.write(text)
