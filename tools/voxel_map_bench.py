"""The sparse voxel map (ndt_map_*) against the batch filter it replaces (tuning aid, not collected by pytest).

    python tools/voxel_map_bench.py              wall times (median of REPS, every call complete when it returns)
    python tools/voxel_map_bench.py --kernels    the same calls a few times, for `rocprofv3 --kernel-trace --stats -- ...`

Steps: (1) one 65 536-point scan into an empty map, (2) the same scan into a map of about 1 M voxels, (3) the export of
that map, (4) a map built from 16 scans.  Yardsticks (ndt_voxel_downsample_device): for an add, the same single scan; for
the build-up, the filter on the 16-scan concatenation plus the time to concatenate, and the filter on the growing
concatenation after every scan (the only way to an intermediate map without ndt_map_*).

Expectation written down before the first run: an add costs no more than about the downsample of the same scan (its key /
sort / run work plus table probes); the 16-scan build-up beats re-filtering the growing concatenation after every scan."""
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
    o = [hip.upload(np.zeros(len(cat), np.float32)) for _ in range(3)]
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    print("scan: %d points, leaf %.2f m, %d repetitions" % (n, LEAF, REPS), flush=True)

    # yardstick of an add: the batch filter on the same scan
    for _ in range(3):
        m1 = ndt.voxelDownsampleDevice(d[0][0], d[0][1], d[0][2], n, LEAF, o[0], o[1], o[2], n)
    t_ds = med(lambda: ndt.voxelDownsampleDevice(d[0][0], d[0][1], d[0][2], n, LEAF, o[0], o[1], o[2], n))
    print("voxelDownsampleDevice, one scan            : %8.3f ms (%d voxels)" % (t_ds, m1), flush=True)

    # (1) one scan into an empty map
    ndt.mapReset(LEAF)
    ndt.mapAddDevice(d[0][0], d[0][1], d[0][2], n)
    t_add0 = med(lambda: ndt.mapAddDevice(d[0][0], d[0][1], d[0][2], n), before=lambda: ndt.mapReset(LEAF))
    print("(1) mapAddDevice into an empty map         : %8.3f ms (mapReset not timed)" % t_add0, flush=True)

    # (2), (3) a map of about 1 M voxels: random points, 6.4 M cells
    rng = np.random.default_rng(0)
    fill = rng.uniform([-100, -100, -10], [100, 100, 10], (1200000, 3)).astype(np.float32)
    ndt.mapReset(LEAF)
    for a in range(0, len(fill), 200000):
        ndt.mapAdd(fill[a:a + 200000])
    info = ndt.mapInfo()
    t_add1 = med(lambda: ndt.mapAddDevice(d[1][0], d[1][1], d[1][2], n))
    print("(2) mapAddDevice into a map of %7d voxels: %8.3f ms (capacity %d)" % (info["n_voxels"], t_add1, info["capacity"]), flush=True)
    nv = ndt.mapInfo()["n_voxels"]
    ox = [hip.upload(np.zeros(nv, np.float32)) for _ in range(3)]
    t_exp = med(lambda: ndt.mapExportDevice(ox[0], ox[1], ox[2], nv))
    print("(3) mapExportDevice of %7d voxels        : %8.3f ms" % (nv, t_exp), flush=True)

    # (4) 16 scans: the map against the filter on the concatenation, once and after every scan
    def build_map():
        ndt.mapReset(LEAF)
        for k in range(16):
            ndt.mapAddDevice(d[k][0], d[k][1], d[k][2], n)
    build_map()
    t_map = med(build_map, reps=max(3, REPS // 3))
    nv16 = ndt.mapInfo()["n_voxels"]
    t_map_exp = med(lambda: ndt.mapExportDevice(o[0], o[1], o[2], len(cat)), reps=max(3, REPS // 3))

    def concat():                                                            # device-to-device, scan by scan
        for k in range(16):
            for a in range(3):
                hip.rt.hipMemcpy(dcat[a] + 4 * n * k, d[k][a], 4 * n, 3)
    t_cat = med(concat, reps=max(3, REPS // 3))
    t_once = med(lambda: ndt.voxelDownsampleDevice(dcat[0], dcat[1], dcat[2], len(cat), LEAF, o[0], o[1], o[2], len(cat)),
                 reps=max(3, REPS // 3))

    def refilter():
        for k in range(16):
            ndt.voxelDownsampleDevice(dcat[0], dcat[1], dcat[2], n * (k + 1), LEAF, o[0], o[1], o[2], len(cat))
    t_re = med(refilter, reps=max(3, REPS // 3))
    print("(4) map from 16 scans (reset + 16 adds)    : %8.3f ms, + one export %.3f ms (%d voxels)" % (t_map, t_map_exp, nv16), flush=True)
    print("    filter on the concatenation, once      : %8.3f ms + %.3f ms to concatenate" % (t_once, t_cat), flush=True)
    print("    filter after every scan (growing cloud): %8.3f ms + %.3f ms to concatenate" % (t_re, t_cat), flush=True)
    print("    16 x (add + export), an intermediate map after every scan: about %.3f ms" % (t_map + 16 * t_map_exp), flush=True)


if __name__ == "__main__":
    main()
