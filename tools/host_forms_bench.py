"""The host forms that cross the host-cloud boundary, timed on the workloads of voxel_map_bench.py, deskew_bench.py and
unproject_bench.py (tuning aid, not collected by pytest): ndt_map_add with intensity, ndt_map_export, ndt_deskew and
ndt_unproject.  Host clock around calls that are complete when they return, profiler off; every row is BLOCKS medians of
REPS calls.

    python tools/host_forms_bench.py                       one process, the library NDT_HIP_LIB names (default: in-tree)
    python tools/host_forms_bench.py --ab A.so B.so [R]    R rounds (default 5) of child processes that alternate between
                                                           the two libraries (A B A B ..., as tools/lib_ab.py does), then
                                                           per row: every number, each process's median, and whether B's
                                                           median of medians is no higher than A's slowest process
                                                           (exit status 1 if a row's is)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
REPS, BLOCKS, WARMUP = 15, 3, 3


def blocks(fn, before=None):
    out = []
    for b in range(BLOCKS):
        ts = []
        for k in range(REPS + (WARMUP if b == 0 else 0)):
            if before:
                before()
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e6)
        out.append(float(np.median(ts[-REPS:])))
    return out


def workload():
    import __graft_entry__ as ge
    import deskew_bench
    import unproject_bench
    pkg = ge.load_package()
    from slam_sam_amd import replay
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    rows = []
    # the voxel map: one 65 536-point scan with an intensity column; the export of a map of random points
    scan, T = next(iter(replay.make_stream(n_frames=1, beams=128, cols=512)))
    scan = pkg.synth.transform(T, scan).astype(np.float32)
    rng = np.random.default_rng(0)
    cloud = np.ascontiguousarray(np.column_stack([scan, rng.uniform(0, 255, len(scan)).astype(np.float32)]))
    rows.append(("ndt_map_add, intensity, %d points" % len(cloud),
                 blocks(lambda: ndt.mapAdd(cloud, intensity_column=3), before=lambda: ndt.mapReset(0.5, with_intensity=True))))
    fill = rng.uniform([-100, -100, -10, 0], [100, 100, 10, 255], (400000, 4)).astype(np.float32)
    ndt.mapReset(0.5, with_intensity=True)
    ndt.mapAdd(fill, intensity_column=3)
    nv = ndt.mapInfo()["n_voxels"]
    rows.append(("ndt_map_export, intensity, %d voxels" % nv, blocks(lambda: ndt.mapExport(columns=4, intensity_column=3))))
    ndt.mapClear()
    # the deskew: 131 072 points, 22 knots, the filter that keeps about half
    pts, inten, alpha, traj, filt = deskew_bench.scan_and_trajectories(pkg)
    kt, kp = traj[22]
    cloud = np.ascontiguousarray(np.column_stack([pts, inten]))
    rows.append(("ndt_deskew, compacting, 22 knots, %d points" % len(cloud),
                 blocks(lambda: ndt.deskew(cloud, alpha, kt, kp, filter=filt, intensity_column=3))))
    # the unprojection: 2048 x 128 pixels, gate, filter, 22 knots
    model, img, gate, filt, kt, kp = unproject_bench.frame(pkg)
    ndt.setScanModel(*model)
    r, refl, t = img["range_mm"], img["reflectivity"], img["col_t"]
    rows.append(("ndt_unproject, compacting, %d pixels" % r.size, blocks(lambda: ndt.unproject(r, refl, t, kt, kp, gate=gate, filter=filt))))
    ndt.close()
    for name, v in rows:
        print("row | %s | %s" % (name, " ".join("%.1f" % x for x in v)), flush=True)


def ab(lib_a, lib_b, rounds):
    got = {}
    for r in range(rounds):
        for which, lib in (("A", lib_a), ("B", lib_b)):
            env = dict(os.environ, NDT_HIP_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=240)
            if p.returncode != 0:   # nothing more is started on the GPU behind a process that failed
                raise SystemExit("host_forms_bench: %s, round %d, exit %d: %s" % (lib, r, p.returncode, p.stderr[-600:]))
            for ln in p.stdout.splitlines():
                if ln.startswith("row | "):
                    _, name, nums = ln.split(" | ")
                    got.setdefault(name, {"A": [], "B": []})[which].append([float(x) for x in nums.split()])
            print("round %d %s done" % (r, which), flush=True)
    print("A = %s\nB = %s\nus per call; %d processes per library, alternating; per process %d medians of %d calls" % (lib_a, lib_b, rounds, BLOCKS, REPS))
    ok = True
    for name, v in got.items():
        med = {w: [float(np.median(run)) for run in v[w]] for w in "AB"}
        b_med, a_max = float(np.median(med["B"])), max(med["A"])
        ok = ok and b_med <= a_max
        print("\n%s" % name)
        for w in "AB":
            print("  %s all   : %s" % (w, "  ".join(" ".join("%.1f" % x for x in run) for run in v[w])))
            print("  %s medians: %s" % (w, " ".join("%.1f" % x for x in med[w])))
        print("  B's median of medians %.1f %s A's slowest process %.1f: %s" % (b_med, "<=" if b_med <= a_max else ">", a_max,
                                                                               "pass" if b_med <= a_max else "FAIL"))
    print("\nall rows pass" if ok else "\na row FAILS")
    return ok


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--ab":
        sys.exit(0 if ab(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 5) else 1)
    else:
        workload()
