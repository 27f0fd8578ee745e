"""Distribution-to-distribution registration of a submap to the map (tuning aid, not collected by pytest).

    python tools/d2d_bench.py [--out FILE] [--small]

Scene: the open-terrain surfaces of synth.config_c3_wide (hills and the vertical faces of 60 buildings on 260 m x 260 m).
The map holds 2 000 000 points at a 1.0 m leaf with moments and becomes the target (ndt_set_target_from_map_moments).  The
submap is ANOTHER sample of the same surfaces, 400 000 points within 70 m of its sensor, accumulated in a frame that is off
by a known pose (0.30 m, 2 degrees); its ndt_map_export_state_device records become the distribution source without
leaving the device.  Reported, every call complete when it returns (host clock around calls that end in a device
synchronise, warmed up, median and spread of the repetitions):
  - microseconds per ndt_eval_derivatives_d2d (K = 1) with and without the Hessian, at the true pose;
  - ndt_align_d2d from the identity guess: iterations, evaluations, milliseconds, distance from the true pose;
  - the route that existed before, on the same handle and the same box: the submap's float centroids (ndt_map_export of
    voxels with at least 6 points) as a point source and ndt_align -- the same figures.
No ratio between the two routes is fixed in advance.  Writes what it prints to profiles/d2d.txt (or --out)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

LEAF = 1.0
KW = dict(resolution=LEAF, step_size=0.1, trans_epsilon=1e-4, max_iterations=35)
TRUE_POSE6 = (0.24, -0.16, 0.08, np.deg2rad(0.9), np.deg2rad(-0.7), np.deg2rad(1.6))
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    ts = np.array(ts)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def main():
    out = os.path.join(ROOT, "profiles", "d2d.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    small = "--small" in sys.argv
    pkg = ge.load_package()
    synth = pkg.synth
    n_map, n_sub = (200000, 40000) if small else (2000000, 400000)
    half = 40.0 if small else 130.0
    reach = 25.0 if small else 70.0
    rng = np.random.default_rng(21)
    nb = 10 if small else 60
    boxes = np.stack([rng.uniform(-half + 10, half - 10, nb), rng.uniform(-half + 10, half - 10, nb), rng.uniform(2.0, 9.0, nb),
                      rng.uniform(2.0, 9.0, nb), rng.uniform(4.0, 12.0, nb)], 1)
    m = synth._wide_surfaces(rng, n_map - n_map // 5, n_map // 5, half, boxes)
    m = (m + rng.normal(0.0, 0.02, m.shape)).astype(np.float32)
    rs = np.random.default_rng(22)
    cand = synth._wide_surfaces(rs, 8 * n_sub, 2 * n_sub, half, boxes)
    cand = cand[np.hypot(cand[:, 0] - 5.0, cand[:, 1] + 3.0) < reach][:n_sub]
    cand = cand + rs.normal(0.0, 0.02, cand.shape)
    truth = synth.pose_matrix(*TRUE_POSE6)
    sub = synth.transform(np.linalg.inv(truth), cand).astype(np.float32)
    assert len(sub) == n_sub

    hip = pkg.ranks.Hip(0)
    A =pkg.NormalDistributionsTransform(device_id=0, **KW)
    A.mapReset(LEAF)
    A.mapEnableMoments()
    A.mapAdd(m)
    A.setInputTargetFromMapMoments()
    B = pkg.NormalDistributionsTransform(device_id=0, **KW)
    B.mapReset(LEAF)
    B.mapEnableMoments()
    B.mapAdd(sub)
    cap = B.mapInfo()["n_voxels"]
    d_ijk, d_cnt = hip.upload(np.zeros((cap, 3), np.int32)), hip.upload(np.zeros(cap, np.int32))
    d_sums, d_mom = hip.upload(np.zeros((cap, 4), np.float32)), hip.upload(np.zeros((cap, 9), np.float64))
    n_rec = B.mapExportStateDevice(d_ijk, d_cnt, d_sums, d_mom, cap)
    t_set = timed(lambda: pkg.setSourceDistributionsDevice(A, d_cnt, d_mom, n_rec), 10)
    n_rec, n_acc = pkg.sourceDistributionsInfo(A)
    gi = A.getGridInfo()
    say("Distribution-to-distribution NDT: a submap's voxels registered to the map's (DESIGN 7l) -- tools/d2d_bench.py")
    say("map: %d points, leaf %.1f m, %d leaves in %d cells; submap: %d points, %d records, %d source Gaussians; DIRECT7"
        % (len(m), LEAF, gi["n_leaves"], gi["n_cells"], len(sub), n_rec, n_acc))
    say("true pose: %.2f m, %.2f deg from the identity guess" % (np.linalg.norm(TRUE_POSE6[:3]), np.rad2deg(np.linalg.norm(TRUE_POSE6[3:]))))
    say("ndt_set_source_distributions_device (records -> Gaussians, awaited): %.3f ms (10 %% %.3f, 90 %% %.3f)"
        % tuple(1e3 * v for v in t_set))
    pose = np.array(TRUE_POSE6)
    e = pkg.evalDerivativesD2D(A, pose)[0]
    say("at the true pose: %d pairs, %d Gaussians with a neighbour" % (e["n_pairs"], e["n_with_neighbors"]))
    for hess in (True, False):
        t = timed(lambda: pkg.evalDerivativesD2D(A, pose, compute_hessian=hess, raw=True), 200, warm=10)
        say("ndt_eval_derivatives_d2d, K = 1, %-20s %8.1f us per evaluation (10 %% %.1f, 90 %% %.1f; launch, sum, read-back and wait included)"
            % ("with the Hessian:" if hess else "without the Hessian:", 1e6 * t[0], 1e6 * t[1], 1e6 * t[2]))

    res = {}

    def run_d2d():
        res["d2d"] = pkg.alignDistributions(A, np.eye(4))

    t = timed(run_d2d, 20)
    T, r = res["d2d"]
    dt, dr = synth.pose_error(T, truth)
    say("ndt_align_d2d:                 %2d iterations, %2d evaluations, %8.3f ms (10 %% %.3f, 90 %% %.3f), %.4f m %.2e rad from the true pose, converged %s"
        % (r["iterations"], r["n_evaluations"], 1e3 * t[0], 1e3 * t[1], 1e3 * t[2], dt, dr, r["converged"]))

    cent = B.mapExport(min_points=6)
    A.setInputSource(cent)

    def run_p2d():
        res["p2d"] = A.align(np.eye(4))

    t = timed(run_p2d, 20)
    r = A.getResult()
    dt, dr = synth.pose_error(res["p2d"], truth)
    say("centroids + ndt_align:         %2d iterations, %2d evaluations, %8.3f ms (10 %% %.3f, 90 %% %.3f), %.4f m %.2e rad from the true pose, converged %s  (%d centroids)"
        % (r["iterations"], r["n_evaluations"], 1e3 * t[0], 1e3 * t[1], 1e3 * t[2], dt, dr, r["converged"], len(cent)))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
