"""Re-posing the voxel map (tuning aid, not collected by pytest).

    python tools/map_repose_bench.py [--out FILE]     wall times (median of REPS, every call complete when it returns)

ndt_map_transform on maps of 2^17 and 2^20 voxels (leaf 0.5 m, two points per voxel), with and without moments, under a
general rigid pose -- against the only route there was before the call existed: ndt_map_export_state to the host, the
per-record rule in NumPy (tests/test_map_repose_cpu.repose_records, the restatement the tests compare with),
ndt_map_reset (+ ndt_map_enable_moments) and ndt_map_import_state.  The three library calls of that route are unchanged by
the re-pose, so they are timed in this library.  The map is refilled before every repetition.
Expectation, written before the first run: the record pass streams about 212 B per voxel with moments (4 B count, 16 B
float sums, 72 B moments, read and written once each, 8 B key, 4 B of statistics traffic amortised) -- 0.22 GB at 2^20
voxels, well under a millisecond at HBM rates; the call is bound by what surrounds it: the fresh table's allocation and
clearing (100 B per slot, 2 slots per voxel), the export's count / compaction / key sort, the import's insert / slot sort /
run search / merge, and three host waits.  No ratio to the host route is fixed in advance.
Writes what it prints to profiles/map_repose.txt (or --out)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

REPS = 5
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
    from test_map_repose_cpu import repose_records, rigid_pose
    out = os.path.join(ROOT, "profiles", "map_repose.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    pkg = ge.load_package()
    hip = pkg.ranks.Hip(0)
    T = rigid_pose()
    say("Re-posing the voxel map (ndt_map_transform; DESIGN 7k) -- tools/map_repose_bench.py")
    say("leaf %.2f m, two points per voxel, rigid pose (yaw 0.3 rad, small roll and pitch, t = (10.3, -4.7, 0.21)), median of %d" % (LEAF, REPS))
    say("host route: ndt_map_export_state -> the rule in NumPy -> ndt_map_reset -> ndt_map_import_state")
    for dims in ((64, 64, 32), (128, 128, 64)):
        nvox = dims[0] * dims[1] * dims[2]
        rng = np.random.default_rng(nvox)
        ijk = np.stack(np.meshgrid(*[np.arange(d) - d // 2 for d in dims], indexing="ij"), axis=-1).reshape(-1, 3)
        pts = ((np.repeat(ijk, 2, axis=0) + rng.uniform(0.05, 0.95, (2 * nvox, 3))) * LEAF).astype(np.float32)
        d = [hip.upload(np.ascontiguousarray(pts[:, a])) for a in range(3)]
        for moments in (True, False):
            ndt = pkg.NormalDistributionsTransform(device_id=0, **KW)

            def fill():
                ndt.mapReset(LEAF)
                if moments:
                    ndt.mapEnableMoments()
                ndt.mapAddDevice(d[0], d[1], d[2], len(pts))

            def host_route():
                st = ndt.mapExportState()
                rec, bad = repose_records(st, T, LEAF)
                assert bad == 0
                ndt.mapReset(LEAF)
                if moments:
                    ndt.mapEnableMoments()
                ndt.mapImportState(leaf=LEAF, ijk=rec["ijk"], count=rec["count"], sums=rec["sums"], moments=rec["moments"])

            fill()
            before = ndt.mapInfo()
            assert before["n_voxels"] == nvox
            t_dev = med(lambda: pkg.mapTransform(ndt, T), before=fill)
            after = ndt.mapInfo()
            t_host = med(host_route, before=fill)
            assert ndt.mapInfo()["n_voxels"] == after["n_voxels"]
            fill()
            t_export = med(ndt.mapExportState)
            say("    %8d voxels, %-15s mapTransform %9.3f ms   host route %10.3f ms (its export alone %9.3f ms)   -> %d voxels in %d slots"
                % (nvox, "with moments" if moments else "without moments", t_dev, t_host, t_export, after["n_voxels"], after["capacity"]))
            ndt.mapClear()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
