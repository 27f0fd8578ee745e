"""The voxel map's crop, state export and state import (tuning aid, not collected by pytest).

    python tools/map_state_bench.py              wall times (median of REPS, every call complete when it returns)
    python tools/map_state_bench.py --kernels    the same calls a few times, for `rocprofv3 --kernel-trace --stats -- ...`

65 536-point scans of the synthetic street, leaf 0.5 m, the 16-scan map of tools/map_target_bench.py (moments on).
(a) mapCrop to the 100 m box around the last pose (the map is refilled before every repetition), the same crop when
    nothing is left to remove (the count pass alone), mapCrop(remove_inside) of the same box; next to them
    mapExportDevice of the same map and one growth of the same table (an add of 131 072 points that has to double the
    table, minus the same add into the table once grown).
(b) mapExportStateDevice of the whole map and of the box; mapImportStateDevice of the whole map's records into an empty map
    and into the 16-scan map (every voxel shared), next to mapAddDevice of as many points; moments on and off.
(c) 16 x (add + crop to the 100 m box around that scan's pose) against 16 adds alone: capacity, voxels, growths, time.

Expectations written down before the first run are in profiles/map_state.txt."""
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
    two = np.concatenate(scans[:2])
    dtwo = [hip.upload(np.ascontiguousarray(two[:, a])) for a in range(3)]
    ndt = pkg.NormalDistributionsTransform(device_id=0, **KW)
    other = pkg.NormalDistributionsTransform(device_id=0, **KW)
    print("scan: %d points, leaf %.2f m, %d repetitions" % (n, LEAF, REPS), flush=True)

    def reset(h, moments, capacity=0):
        h.mapReset(LEAF, initial_capacity=capacity)
        if moments:
            h.mapEnableMoments()

    def fill(h=ndt, moments=True, upto=16):
        reset(h, moments)
        for k in range(upto):
            h.mapAddDevice(d[k][0], d[k][1], d[k][2], n)

    def box(k, half=50.0):
        c = stream[k][1][:3, 3]
        return (c - half).astype(np.float32), (c + half).astype(np.float32)

    # (a) crop, next to the export and one growth of the same table
    lo, hi = box(15)
    fill()
    info = ndt.mapInfo()
    inside = len(ndt.mapExportState(lo, hi)["count"])
    print("(a) the 16-scan map: %d voxels in %d slots, %d of them inside the 100 m box" % (info["n_voxels"], info["capacity"], inside),
          flush=True)
    t_crop = med(lambda: ndt.mapCrop(lo, hi), before=fill)
    cap_after = ndt.mapInfo()["capacity"]
    t_noop = med(lambda: ndt.mapCrop(lo, hi))
    t_erase = med(lambda: ndt.mapCrop(lo, hi, remove_inside=True), before=fill)
    fill()
    o = [hip.upload(np.zeros(info["n_voxels"], np.float32)) for _ in range(3)]
    ndt.mapExportDevice(o[0], o[1], o[2], info["n_voxels"])
    t_export = med(lambda: ndt.mapExportDevice(o[0], o[1], o[2], info["n_voxels"]))
    t_grow = med(lambda: ndt.mapAddDevice(dtwo[0], dtwo[1], dtwo[2], 2 * n), before=fill)
    grown = ndt.mapInfo()
    t_grown = med(lambda: ndt.mapAddDevice(dtwo[0], dtwo[1], dtwo[2], 2 * n))
    assert grown["n_grows"] == 1 and grown["capacity"] == 2 * info["capacity"] and ndt.mapInfo()["n_grows"] == 1
    print("    mapCrop to the box                 %8.3f ms (capacity afterwards %d)" % (t_crop, cap_after), flush=True)
    print("    mapCrop, nothing left to remove    %8.3f ms" % t_noop, flush=True)
    print("    mapCrop(remove_inside) of the box  %8.3f ms" % t_erase, flush=True)
    print("    mapExportDevice of the same map    %8.3f ms" % t_export, flush=True)
    print("    one growth of the same table       %8.3f ms (add of %d points with the growth %.3f, without %.3f)"
          % (t_grow - t_grown, 2 * n, t_grow, t_grown), flush=True)

    # (b) the state out and back in
    for moments in (True, False):
        tag = "on " if moments else "off"
        fill(moments=moments)
        m = ndt.mapInfo()["n_voxels"]
        s_ijk, s_cnt = hip.upload(np.zeros((m, 3), np.int32)), hip.upload(np.zeros(m, np.int32))
        s_sum = hip.upload(np.zeros((m, 4), np.float32))
        s_mom = hip.upload(np.zeros((m, 9), np.float64)) if moments else None
        assert ndt.mapExportStateDevice(s_ijk, s_cnt, s_sum, s_mom, m) == m
        t_xs = med(lambda: ndt.mapExportStateDevice(s_ijk, s_cnt, s_sum, s_mom, m))
        t_xb = med(lambda: ndt.mapExportStateDevice(s_ijk, s_cnt, s_sum, s_mom, m, lo, hi))
        assert ndt.mapExportStateDevice(s_ijk, s_cnt, s_sum, s_mom, m) == m       # (the whole map's records again)
        t_i0 = med(lambda: other.mapImportStateDevice(LEAF, s_ijk, s_cnt, s_sum, s_mom, m), before=lambda: reset(other, moments))
        assert other.mapInfo()["n_voxels"] == m
        t_a0 = med(lambda: other.mapAddDevice(d[3][0], d[3][1], d[3][2], m), before=lambda: reset(other, moments))
        fill(other, moments)
        t_i1 = med(lambda: other.mapImportStateDevice(LEAF, s_ijk, s_cnt, s_sum, s_mom, m))
        assert other.mapInfo()["n_voxels"] == m
        t_a1 = med(lambda: other.mapAddDevice(d[3][0], d[3][1], d[3][2], m))
        print("(b) moments %s, %d records: export state %8.3f ms (box %8.3f) | import into an empty map %8.3f ms (add of %d points "
              "%8.3f) | into the 16-scan map %8.3f ms (add %8.3f)" % (tag, m, t_xs, t_xb, t_i0, m, t_a0, t_i1, t_a1), flush=True)

    # (c) the sliding window
    def drive(crop, report=False):
        reset(ndt, True)
        for k in range(16):
            ndt.mapAddDevice(d[k][0], d[k][1], d[k][2], n)
            if crop:
                ndt.mapCrop(*box(k))
            if report:
                i = ndt.mapInfo()
                print("      scan %2d: %6d voxels, capacity %7d, %d growths" % (k, i["n_voxels"], i["capacity"], i["n_grows"]), flush=True)

    for crop in (False, True):
        print("(c) 16 x %s" % ("(add + crop to the 100 m box)" if crop else "add"), flush=True)
        drive(crop, report=True)
        print("    %8.3f ms for the 16 scans" % med(lambda: drive(crop), reps=max(3, REPS // 3)), flush=True)


if __name__ == "__main__":
    main()
