"""Connected components of the voxel map (tuning aid, not collected by pytest).

    python tools/map_components_bench.py [--out FILE]   wall times (median of REPS, every call complete when it returns)
    python tools/map_components_bench.py --kernels      the same calls a few times, for `rocprofv3 --kernel-trace --stats -- ...`
                                                        (k_mapcc_link alone is read from that run's statistics)

The C3 map (synth.config_c3: a million points of eight scans along a track) is accumulated as a voxel map at leaf 0.5 m.
Timed: ndt_map_components per connectivity (a one-point ndt_map_add in front of every repetition, outside the timing,
makes the cached labelling stale), ndt_map_label_points_device for C3's 200 000-point scan under its pose (the labelling
is cached: one launch and one wait), one ndt_map_remove_components(min_voxels = 3) for real (the map is refilled in front
of every repetition; labelling and move are inside the timing) -- and, as the yardstick, ndt_map_export_state of the
same map: what a host-side labelling would have to pay before it starts.
Writes what it prints to profiles/map_components.txt (or --out)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

KERNELS = "--kernels" in sys.argv
REPS = 3 if KERNELS else 20
LEAF = 0.5
KW = dict(resolution=LEAF, step_size=0.1, trans_epsilon=1e-4, max_iterations=35)
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def med(fn, reps=REPS, before=None):
    ts = []
    for _ in range(reps):
        if before:
            before()
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def main():
    out = os.path.join(ROOT, "profiles", "map_components.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    pkg = ge.load_package()
    hip = pkg.ranks.Hip(0)
    cfg = pkg.synth.config_c3()
    tgt = np.ascontiguousarray(cfg["target"][:, :3], np.float32)
    src = np.ascontiguousarray(cfg["source"][:, :3], np.float32)
    pose = np.asarray(cfg["gt"], np.float64)
    d_tgt = [hip.upload(np.ascontiguousarray(tgt[:, a])) for a in range(3)]
    d_src = [hip.upload(np.ascontiguousarray(src[:, a])) for a in range(3)]
    d_lab = hip.upload(np.zeros(len(src), np.int32))
    ndt = pkg.NormalDistributionsTransform(device_id=0, **KW)
    one = tgt[:1].copy()

    def fill():
        ndt.mapReset(LEAF)
        ndt.mapEnableMoments()
        ndt.mapAddDevice(d_tgt[0], d_tgt[1], d_tgt[2], len(tgt))

    fill()
    info = ndt.mapInfo()
    say("Connected components of the voxel map (ndt_map_components*; DESIGN 7r) -- tools/map_components_bench.py")
    say("map: C3's %d points at leaf %.2f m: %d voxels in %d slots, moments on; median of %d" % (len(tgt), LEAF, info["n_voxels"],
                                                                                             info["capacity"], REPS))
    for c in (6, 18, 26):
        say("    connectivity %2d: %s" % (c, pkg.mapComponents(ndt, c)))
    stale = lambda: ndt.mapAdd(one)
    t_cc = {c: med(lambda: pkg.mapComponents(ndt, c), before=stale) for c in (6, 18, 26)}
    pkg.mapComponents(ndt, 26)
    labelled = pkg.mapLabelPointsDevice(ndt, d_src[0], d_src[1], d_src[2], len(src), d_lab, pose=pose)
    t_pts = med(lambda: pkg.mapLabelPointsDevice(ndt, d_src[0], d_src[1], d_src[2], len(src), d_lab, pose=pose))
    fill()
    removed = pkg.mapRemoveComponents(ndt, 26, min_voxels=3, dry_run=True)
    t_rm = med(lambda: pkg.mapRemoveComponents(ndt, 26, min_voxels=3), before=fill)
    fill()
    t_state = med(lambda: ndt.mapExportState())
    for c in (6, 18, 26):
        say("    mapComponents          connectivity %2d          %9.3f ms" % (c, t_cc[c]))
    say("    mapLabelPointsDevice   %d points, cached labels  %9.3f ms   (%d labelled)" % (len(src), t_pts, labelled))
    say("    mapRemoveComponents    min_voxels 3, for real    %9.3f ms   %s" % (t_rm, removed))
    say("    mapExportState         the yardstick             %9.3f ms" % t_state)
    if not KERNELS:
        with open(out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
