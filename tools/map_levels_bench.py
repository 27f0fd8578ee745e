"""The voxel map's levels: deriving them, a level as the target, coarse-to-fine alignment (tuning aid, not
collected by pytest).

    python tools/map_levels_bench.py [--out FILE] [--small]

Scene: the map of tools/d2d_bench.py -- the open-terrain surfaces of synth.config_c3_wide, 2 000 000 points at a 1.0 m leaf
with moments.  The source of the aligns is another sample of the surfaces, 40 000 points within 70 m of its sensor, in a
frame that is off by a known pose (1.1 m, 3 degrees: outside the 1 m leaf's basin).  Reported, every call complete when it
returns (host clock around calls that end in a device synchronise, warmed up, median and 10th / 90th percentile of the
repetitions):
  - deriving level 1, 2 and 3 (ndt_map_levels_drop, untimed, then ndt_map_level_info);
  - ndt_set_target_from_map_level with the level cached, and stale (dropped before every call);
  - the only route there was before, per level: ndt_map_export_state to the host, ijk >> L there, ndt_map_import_state
    into a second handle's fresh map of leaf * 2^L, ndt_set_target_from_map_moments there;
  - ndt_align_map_levels [2, 1, 0] and the fine-only align from the same guess: milliseconds, distance from the true pose.
No ratio between the routes is fixed in advance.  Writes what it prints to profiles/map_levels.txt (or --out)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

LEAF = 1.0
KW = dict(resolution=LEAF, step_size=0.1, trans_epsilon=1e-4, max_iterations=35)
TRUE_POSE6 = (0.9, -0.6, 0.1, np.deg2rad(0.5), np.deg2rad(-0.4), np.deg2rad(2.9))
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed(fn, reps, warm=2, before=None):
    """median, 10th and 90th percentile of fn's wall time in ms; `before` runs untimed in front of every call"""
    ts = []
    for k in range(warm + reps):
        if before:
            before()
        t = time.perf_counter()
        fn()
        if k >= warm:
            ts.append(time.perf_counter() - t)
    ts = 1e3 * np.array(ts)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def main():
    out = os.path.join(ROOT, "profiles", "map_levels.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    small = "--small" in sys.argv
    pkg = ge.load_package()
    synth = pkg.synth
    n_map, n_src = (200000, 8000) if small else (2000000, 40000)
    half = 40.0 if small else 130.0
    reach = 25.0 if small else 70.0
    reps = 5 if small else 15
    rng = np.random.default_rng(21)
    nb = 10 if small else 60
    boxes = np.stack([rng.uniform(-half + 10, half - 10, nb), rng.uniform(-half + 10, half - 10, nb), rng.uniform(2.0, 9.0, nb),
                      rng.uniform(2.0, 9.0, nb), rng.uniform(4.0, 12.0, nb)], 1)
    m = synth._wide_surfaces(rng, n_map - n_map // 5, n_map // 5, half, boxes)
    m = (m + rng.normal(0.0, 0.02, m.shape)).astype(np.float32)
    rs = np.random.default_rng(22)
    cand = synth._wide_surfaces(rs, 80 * n_src, 20 * n_src, half, boxes)
    cand = cand[np.hypot(cand[:, 0] - 5.0, cand[:, 1] + 3.0) < reach][:n_src]
    cand = cand + rs.normal(0.0, 0.02, cand.shape)
    truth = synth.pose_matrix(*TRUE_POSE6)
    src = synth.transform(np.linalg.inv(truth), cand).astype(np.float32)
    assert len(src) == n_src

    A = pkg.NormalDistributionsTransform(device_id=0, **KW)
    A.mapReset(LEAF)
    A.mapEnableMoments()
    A.mapAdd(m)
    A.setInputSource(src)
    B = pkg.NormalDistributionsTransform(device_id=0, **KW)
    info = A.mapInfo()
    say("Voxel-map levels: coarser targets from the map's own sums (DESIGN 7n) -- tools/map_levels_bench.py")
    say("map: %d points, leaf %.1f m, %d voxels in %d table slots, moments on; %d repetitions per figure, ms: median (10 %%, 90 %%)"
        % (len(m), LEAF, info["n_voxels"], info["capacity"], reps))
    say("%-7s %-9s %-9s | %-26s | %-26s %-26s | %-26s" % ("level", "leaf", "voxels", "derive", "target, level cached", "target, level stale",
                                                         "host route (export, shift, import, target)"))
    for L in (1, 2, 3):
        leaf_l = LEAF * 2 ** L
        t_derive = timed(lambda: pkg.mapLevelInfo(A, L), reps, before=lambda: pkg.mapLevelsDrop(A))
        li = pkg.mapLevelInfo(A, L)
        A.setParams(resolution=leaf_l)
        t_cached = timed(lambda: pkg.setInputTargetFromMapLevel(A, L), reps)
        t_stale = timed(lambda: pkg.setInputTargetFromMapLevel(A, L), reps, before=lambda: pkg.mapLevelsDrop(A))
        n_leaves = A.getGridInfo()["n_leaves"]
        A.setParams(resolution=LEAF)
        B.setParams(resolution=leaf_l)

        def host_route():
            st = A.mapExportState()
            st["ijk"] = st["ijk"] >> L
            st["leaf"] = leaf_l
            B.mapReset(leaf_l)
            B.mapEnableMoments()
            B.mapImportState(st)
            B.setInputTargetFromMapMoments()

        t_host = timed(host_route, max(3, reps // 3), warm=1)
        assert B.getGridInfo()["n_leaves"] == n_leaves and B.mapInfo()["n_voxels"] == li["n_voxels"]
        fmt = "%8.3f (%8.3f, %8.3f)"
        say("%-7d %-9.1f %-9d | %s | %s %s | %s   %d leaves" % (L, leaf_l, li["n_voxels"], fmt % t_derive, fmt % t_cached, fmt % t_stale,
                                                                 fmt % t_host, n_leaves))
    B.mapClear()

    res = {}

    def run_levels():
        res["levels"] = pkg.alignMapLevels(A, [2, 1, 0], np.eye(4))

    def run_fine():
        res["fine"] = pkg.alignMapLevels(A, [0], np.eye(4))

    say("true pose: %.2f m, %.2f deg from the identity guess; source: %d points" % (np.linalg.norm(TRUE_POSE6[:3]),
                                                                                  np.rad2deg(np.linalg.norm(TRUE_POSE6[3:])), len(src)))
    for name, fn, key in (("ndt_align_map_levels [2, 1, 0], levels cached:", run_levels, "levels"),
                          ("ndt_align_map_levels [0] (fine only):", run_fine, "fine")):
        t = timed(fn, reps)
        r = res[key]
        dt, dr = synth.pose_error(r[-1]["T"], truth)
        say("%-48s %8.3f ms (%.3f, %.3f), iterations %s, %.4f m %.2e rad from the true pose, converged %s"
            % (name, t[0], t[1], t[2], "+".join(str(x["iterations"]) for x in r), dt, dr, r[-1]["converged"]))
    t = timed(run_levels, max(3, reps // 3), warm=1, before=lambda: pkg.mapLevelsDrop(A))
    say("%-48s %8.3f ms (%.3f, %.3f)" % ("ndt_align_map_levels [2, 1, 0], levels stale:", t[0], t[1], t[2]))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
