"""Free-space carving of the voxel map (tuning aid, not collected by pytest).

    python tools/map_carve_bench.py [--out FILE]     wall times (median of REPS, every call complete when it returns)
    python tools/map_carve_bench.py --kernels        the same calls a few times, for `rocprofv3 --kernel-trace --stats -- ...`

One 2048 x 128-pixel scan (262 144 rays) of the synthetic street is carved into a map of about a million voxels at leaf
0.5 m: four such scans under their poses plus uniform clutter in the box around them, so that the rays have something to
cross.  Reported: the three forms of the carve (host cloud, device arrays, archived keyframe) as dry runs -- the traversal
and the count pass, the map unchanged -- and the device form for real (the map is refilled before every repetition, so
the move to a fresh table is included), n_steps per second of the device form's dry run, and for scale ndt_map_add of
the same scan and ndt_map_crop of the same map to the 100 m box around the scan's pose.
Writes what it prints to profiles/map_carve.txt (or --out)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

KERNELS = "--kernels" in sys.argv
REPS = 3 if KERNELS else 11
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
    out = os.path.join(ROOT, "profiles", "map_carve.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    pkg = ge.load_package()
    from slam_sam_amd import replay
    hip = pkg.ranks.Hip(0)
    stream = replay.make_stream(n_frames=4, beams=128, cols=2048)           # 4 scans of 262 144 points, sensor frame
    scans = [np.ascontiguousarray(s[:, :3], np.float32) for s, _ in stream]
    poses = [np.asarray(T, np.float64) for _, T in stream]
    n = len(scans[0])
    # clutter: 1.2 M points in a 260 x 120 x 16 m box around the track (4 M voxels of 0.5 m: about a million occupied)
    c = poses[3][:3, 3]
    rng = np.random.default_rng(1)
    clutter = rng.uniform(c + [-130.0, -60.0, -2.0], c + [130.0, 60.0, 14.0], (1_200_000, 3)).astype(np.float32)
    d_scans = [[hip.upload(np.ascontiguousarray(s[:, a])) for a in range(3)] for s in scans]
    d_clutter = [hip.upload(np.ascontiguousarray(clutter[:, a])) for a in range(3)]
    ndt = pkg.NormalDistributionsTransform(device_id=0, **KW)
    origin = [0.0, 0.0, 0.0]
    scan, pose, d = scans[3], poses[3], d_scans[3]
    ndt.putKeyframe(1, scan)

    def fill():
        ndt.mapReset(LEAF, initial_capacity=1 << 22)
        ndt.mapEnableMoments()
        for k in range(4):
            ndt.mapAddDevice(d_scans[k][0], d_scans[k][1], d_scans[k][2], n, pose=poses[k])
        ndt.mapAddDevice(d_clutter[0], d_clutter[1], d_clutter[2], len(clutter))

    fill()
    info = ndt.mapInfo()
    say("Free-space carving of the voxel map (ndt_map_carve*; DESIGN 7i) -- tools/map_carve_bench.py")
    say("scan: %d rays (2048 x 128), leaf %.2f m, default parameters (min_misses 2, keep_last 1, max_steps 4096), median of %d"
        % (n, LEAF, REPS))
    say("map: %d voxels, %d points, %d slots, moments on" % (info["n_voxels"], info["n_points"], info["capacity"]))
    dry = ndt.mapCarveDevice(d[0], d[1], d[2], n, origin, pose=pose, dry_run=True)
    say("one carve: %s" % dry)
    t_host = med(lambda: ndt.mapCarve(scan, origin, pose=pose, dry_run=True))
    t_dev = med(lambda: ndt.mapCarveDevice(d[0], d[1], d[2], n, origin, pose=pose, dry_run=True))
    t_kf = med(lambda: ndt.mapCarveKeyframe(1, origin, pose, dry_run=True))
    t_real = med(lambda: ndt.mapCarveDevice(d[0], d[1], d[2], n, origin, pose=pose), before=fill)
    after = ndt.mapInfo()
    fill()
    t_add = med(lambda: ndt.mapAddDevice(d[0], d[1], d[2], n, pose=pose))
    box = ((c - 50.0).astype(np.float32), (c + 50.0).astype(np.float32))
    t_crop = med(lambda: ndt.mapCrop(*box), before=fill)
    say("    mapCarve          host cloud, dry run      %9.3f ms" % t_host)
    say("    mapCarveDevice    device arrays, dry run   %9.3f ms   %.3g voxel steps / s" % (t_dev, dry["n_steps"] / (1e-3 * t_dev)))
    say("    mapCarveKeyframe  archived scan, dry run   %9.3f ms" % t_kf)
    say("    mapCarveDevice    for real                 %9.3f ms   (%d voxels left in %d slots)"
        % (t_real, after["n_voxels"], after["capacity"]))
    say("    mapAddDevice      the same scan            %9.3f ms" % t_add)
    say("    mapCrop           100 m box, same map      %9.3f ms" % t_crop)
    if not KERNELS:
        with open(out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
