"""The voxel map's moments and the target made from them (tuning aid, not collected by pytest).

    python tools/map_target_bench.py              wall times (median of REPS, every call complete when it returns)
    python tools/map_target_bench.py --kernels    the same calls a few times, for `rocprofv3 --kernel-trace --stats -- ...`

65 536-point scans of the synthetic street, leaf 0.5 m (as tools/voxel_map_bench.py).
(b) mapAddDevice with moments off and on: into an empty map, into a 16-scan map, and a crowded scan (every point in
    64 voxels: 1024 points per run).
(c) a 16-scan map: setInputTargetFromMapMoments (whole map, 100 m box) against setInputTargetFromMap (centroids) on the
    same map and setInputTargetDevice on the concatenation.
(d) the stream: per scan add + boxed target from moments + align, against add + setInputTargetDevice(concatenation so
    far) + align.

Expectations written down before the first run are in profiles/map_target.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

KERNELS = "--kernels" in sys.argv
REPS = 3 if KERNELS else 15
LEAF = 0.5
KW = dict(resolution=LEAF, step_size=0.1, trans_epsilon=1e-4, max_iterations=35)


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
    pkg = ge.load_package()
    from slam_sam_amd import replay
    hip = pkg.ranks.Hip(0)
    stream = replay.make_stream(n_frames=16, beams=128, cols=512)          # 16 scans of 65 536 points
    scans = [pkg.synth.transform(T, s).astype(np.float32) for s, T in stream]
    n = len(scans[0])
    d = [[hip.upload(np.ascontiguousarray(s[:, a])) for a in range(3)] for s in scans]
    cat = np.concatenate(scans)
    dcat = [hip.upload(np.ascontiguousarray(cat[:, a])) for a in range(3)]
    rng = np.random.default_rng(1)
    crowd = (rng.integers(0, 8, (n, 3)) * LEAF + rng.uniform(0.05, 0.45, (n, 3))).astype(np.float32)
    crowd[:, 2] = rng.uniform(0.05, 0.45, n)                                # 8 x 8 x 1 voxels
    dcrowd = [hip.upload(np.ascontiguousarray(crowd[:, a])) for a in range(3)]
    ndt = pkg.NormalDistributionsTransform(device_id=0, **KW)
    print("scan: %d points, leaf %.2f m, %d repetitions" % (n, LEAF, REPS), flush=True)

    def reset(moments):
        ndt.mapReset(LEAF)
        if moments:
            ndt.mapEnableMoments()

    def fill(moments, upto=16):
        reset(moments)
        for k in range(upto):
            ndt.mapAddDevice(d[k][0], d[k][1], d[k][2], n)

    # (b) the add, moments off / on
    for moments in (False, True):
        tag = "on " if moments else "off"
        fill(moments, 1)
        t0 = med(lambda: ndt.mapAddDevice(d[0][0], d[0][1], d[0][2], n), before=lambda: reset(moments))
        fill(moments)
        t1 = med(lambda: ndt.mapAddDevice(d[1][0], d[1][1], d[1][2], n))
        nv = ndt.mapInfo()["n_voxels"]
        reset(moments)
        ndt.mapAddDevice(dcrowd[0], dcrowd[1], dcrowd[2], n)
        t2 = med(lambda: ndt.mapAddDevice(dcrowd[0], dcrowd[1], dcrowd[2], n))
        print("(b) moments %s: add into an empty map %8.3f ms | into the 16-scan map (%d voxels) %8.3f ms | crowded scan "
              "(%d voxels) %8.3f ms" % (tag, t0, nv, t1, ndt.mapInfo()["n_voxels"], t2), flush=True)

    # (c) targets from a 16-scan map
    fill(True)
    c = stream[15][1][:3, 3]
    lo, hi = (c - [50.0, 50.0, 50.0]).astype(np.float32), (c + [50.0, 50.0, 50.0]).astype(np.float32)
    ndt.setInputTargetFromMapMoments()
    t_whole = med(ndt.setInputTargetFromMapMoments)
    g_whole = ndt.getGridInfo()
    ndt.setInputTargetFromMapMoments(lo, hi)
    t_box = med(lambda: ndt.setInputTargetFromMapMoments(lo, hi))
    g_box = ndt.getGridInfo()

    def centroids():
        ndt.setInputTargetFromMap(1)
        ndt.wait()
    centroids()
    t_cent = med(centroids)
    g_cent = ndt.getGridInfo()
    ndt.setInputTargetDevice(dcat[0], dcat[1], dcat[2], len(cat))
    t_dev = med(lambda: ndt.setInputTargetDevice(dcat[0], dcat[1], dcat[2], len(cat)))
    g_dev = ndt.getGridInfo()
    for name, t, g in (("setInputTargetFromMapMoments, whole map ", t_whole, g_whole),
                       ("setInputTargetFromMapMoments, 100 m box ", t_box, g_box),
                       ("setInputTargetFromMap (centroids)       ", t_cent, g_cent),
                       ("setInputTargetDevice(concatenation)     ", t_dev, g_dev)):
        print("(c) %s: %8.3f ms (%d leaves, %d cells, %d points)" % (name, t, g["n_leaves"], g["n_cells"], g["n_target_points"]),
              flush=True)

    # (d) the stream: scan k is registered against the map of scans 0 .. k - 1, then added
    src = [[hip.upload(np.ascontiguousarray(s[:, a].astype(np.float32))) for a in range(3)] for s, _ in stream]
    guesses = [pkg.ColMajor4f(T) for _, T in stream]

    def stream_moments():
        reset(True)
        ndt.mapAddDevice(d[0][0], d[0][1], d[0][2], n)
        for k in range(1, 16):
            ck = stream[k][1][:3, 3]
            ndt.setInputTargetFromMapMoments((ck - 50.0).astype(np.float32), (ck + 50.0).astype(np.float32))
            ndt.setInputSourceDeviceView(src[k][0], src[k][1], src[k][2], n)
            ndt.align(guesses[k], return_transform=False)
            ndt.mapAddDevice(d[k][0], d[k][1], d[k][2], n)

    def stream_concat():
        reset(False)
        ndt.mapAddDevice(d[0][0], d[0][1], d[0][2], n)
        for k in range(1, 16):
            ndt.setInputTargetDevice(dcat[0], dcat[1], dcat[2], n * k)
            ndt.setInputSourceDeviceView(src[k][0], src[k][1], src[k][2], n)
            ndt.align(guesses[k], return_transform=False)
            ndt.mapAddDevice(d[k][0], d[k][1], d[k][2], n)
    stream_moments()
    it_m = ndt.getResult()["iterations"]
    t_sm = med(stream_moments, reps=max(3, REPS // 3))
    stream_concat()
    it_c = ndt.getResult()["iterations"]
    t_sc = med(stream_concat, reps=max(3, REPS // 3))
    print("(d) 15 x (boxed target from moments + align + add): %8.3f ms (last align %d iterations)" % (t_sm, it_m), flush=True)
    print("    15 x (target from the concatenation + align + add): %8.3f ms (last align %d iterations)" % (t_sc, it_c), flush=True)


if __name__ == "__main__":
    main()
