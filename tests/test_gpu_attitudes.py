"""Evaluation, transform, per-point paths, align, batched align and SVN at attitudes all over SO(3).

Every other GPU test evaluates within 0.15 rad of the identity, where two of the three sines are below 1e-2 and most of
j_ang / h_ang is at 1e-2 .. 1e-5 of its full size.  Here the project's two smallest scenes (C1, golden g1) are seen from
the attitudes of tests/test_attitudes_cpu.py -- general, yaw wrap, gimbal corner, both branches of matrix_to_pose's fold,
both sides of the 1e-7 angle snap -- and every path is held to the bounds it already has near the identity:
pair counts exact, score / NVTL / Hessian 1e-9, gradient 1e-9 of the largest norm compared, against the oracle's f64
statement; packed records at test_packed_voxel_records' bounds; transforms bit for bit against the f32 restatement;
aligns within 1 mm / 0.1 mrad of the oracle with every evaluation of the trajectory replayed.  No tolerance is new."""
import numpy as np
import pytest

from test_attitudes_cpu import (ALIGN, ATTITUDES, GENERAL, KW, ORACLE_THREADS, PI, SCENES, base_scene, oracle_grid, scene,
                                scene_at)
from test_gpu_align_batch import _assert_same, _serial
from test_gpu_fitness import check_pose
from test_gpu_launch_shapes import _nbs, bits, compare, words_of
from test_gpu_map_paths import f32_transform
from test_gpu_parity import ALIGN_TOL_M, ALIGN_TOL_RAD
from test_gpu_point_scores import check_sums, per_point_case
from test_gpu_trajectory import _distinct_poses, _oracle_trajectory

pytestmark = pytest.mark.gpu

NB_NAMES = ("DIRECT1", "DIRECT7", "KDTREE", "DIRECT26", "DIRECT1-packed48", "DIRECT7-packed48")
_memo = {}


def oracle_eval(O, name, omethod, att, need_h):
    """the oracle's f64 statement (pair_mode 2) of the evaluation at an attitude's own pose, kept for the record formats
    that share it"""
    k = (name, omethod, att, need_h)
    if k not in _memo:
        s = scene(name, att)
        prm = O.default_params(num_threads=ORACLE_THREADS, pair_mode=2, search_method=omethod, **KW)
        _memo[k] = oracle_grid(name).derivatives(s["source"], s["pose6"], compute_hessian=need_h, params=prm)
    return _memo[k]


def engine(pkg, name, method=None, fmt=None):
    n, info = pkg.backend_info()
    assert n > 0, "GPU test on a box without a HIP device: " + info
    ndt = pkg.NormalDistributionsTransform(device_id=0, **KW)
    if method is not None:
        ndt.setParams(search_method=method)
        ndt.setRecordFormat(fmt)
    ndt.setInputTarget(scene(name, "general-a")["target"])
    return ndt


def compare_packed(got, ref, what):
    """packed 48-byte records (test_gpu_launch_shapes._modes_matrix): the inverse covariance rounded to f32"""
    assert got["n_pairs"] == ref["n_pairs"], what
    assert got["n_with_neighbors"] == ref["n_with_neighbors"], what
    assert got["score"] == pytest.approx(ref["score"], rel=1e-6), what
    assert np.linalg.norm(got["gradient"] - ref["gradient"]) <= 2e-6 * np.linalg.norm(ref["gradient"]) + 1e-9, what


# ---------------------------------------------------------------------------------------- 1. evaluation parity
@pytest.mark.parametrize("nb", range(6), ids=NB_NAMES)
@pytest.mark.parametrize("name", SCENES)
def test_evaluation_at_every_attitude(pkg, O, name, nb):
    """ndt_eval_derivatives from poses6 (the engine builds the f32 matrix and the tables itself), with and without the
    Hessian, at every attitude of the table."""
    method, fmt, omethod, _ = _nbs(pkg, O)[nb]
    ndt = engine(pkg, name, method, fmt)
    try:
        runs = []
        for att in ATTITUDES:
            s = scene(name, att)
            ndt.setInputSource(s["source"])
            for need_h in (True, False):
                got = ndt.evalDerivatives(s["pose6"], compute_hessian=need_h)[0]
                runs.append((att, need_h, got, oracle_eval(O, name, omethod, att, need_h)))
        gscale = max(np.linalg.norm(ref["gradient"]) for _, _, _, ref in runs)
        # (no case compares zeros: at least half the pairs of the unrotated guess, in this neighbourhood too)
        b = base_scene(name)
        n0 = oracle_grid(name).derivatives(b["source"], O.matrix_to_pose(b["guess"]), T=b["guess"], compute_hessian=False,
                                           params=O.default_params(num_threads=ORACLE_THREADS, search_method=omethod, **KW))["n_pairs"]
        assert n0 > 0 and 2 * min(ref["n_pairs"] for _, _, _, ref in runs) >= n0, n0
        failed = []
        for att, need_h, got, ref in runs:
            what = (name, NB_NAMES[nb], att, "H" if need_h else "no H")
            w = {}
            try:
                if nb >= 4:
                    compare_packed(got, ref, what)
                    w = dict(score=abs(got["score"] - ref["score"]) / abs(ref["score"]),
                             g=np.linalg.norm(got["gradient"] - ref["gradient"]) / np.linalg.norm(ref["gradient"]), H=0.0)
                else:
                    compare(got, ref, gscale, need_h, what, worst=w)
            except AssertionError as e:
                failed.append((what, str(e)[:300]))
            if need_h:
                print("ATT %-4s %-16s %-18s pairs %6d  score %.1e  g %.1e  H %.1e" %
                      (name, NB_NAMES[nb], att, ref["n_pairs"], w.get("score", -1), w.get("g", -1), w.get("H", -1)))
        assert not failed, failed
    finally:
        ndt.close()


@pytest.mark.parametrize("nb", range(6), ids=NB_NAMES)
def test_all_attitudes_in_one_batch_are_their_single_pose_calls(pkg, O, nb):
    """One source, every attitude of the table as one batched launch: each pose's 32 words are the words of its own
    K = 1 call, bit for bit (the partition of 10 k points does not depend on K)."""
    method, fmt, _, _ = _nbs(pkg, O)[nb]
    ndt = engine(pkg, "c1", method, fmt)
    try:
        s = scene("c1", "general-a")
        ndt.setInputSource(s["source"])
        poses = np.stack([scene("c1", att)["pose6"] for att in ATTITUDES])
        assert pkg.debug_launch_shape(len(s["source"]), len(poses))[0] == pkg.debug_launch_shape(len(s["source"]), 1)[0]
        for need_h in (True, False):
            ndt.debugEvalLog(2 * len(poses))
            ndt.evalDerivatives(poses, compute_hessian=need_h)
            for p in poses:
                ndt.evalDerivatives(p, compute_hessian=need_h)
            log = ndt.debugEvalLogRead()
            ndt.debugEvalLog(0)
            many, one = log[:len(poses)], log[len(poses):]
            assert len(one) == len(poses) and int(one[0]["words"][30]) > 500       # (general-a is the first of the table)
            for att, a, b in zip(ATTITUDES, many, one):
                assert a["K"] == len(poses) and b["K"] == 1 and np.array_equal(a["T32"], b["T32"]), att
                assert np.array_equal(bits(a["words"]), bits(b["words"])), (NB_NAMES[nb], att, need_h)
    finally:
        ndt.close()


# ---------------------------------------------------------------------------------------- 2. transform and per-point paths
@pytest.mark.parametrize("name", SCENES)
def test_transform_source_at_every_attitude(pkg, name):
    """ndt_transform_source with nine mid-sized rotation entries: x' = r0 x + (r1 y + (r2 z + t)) in f32, never fused."""
    ndt = engine(pkg, name)
    try:
        for att in ATTITUDES:
            s = scene(name, att)
            ndt.setInputSource(s["source"])
            got = ndt.transformSource(s["P"])
            want = f32_transform(s["P"], s["source"])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (att, np.abs(got - want).max())
    finally:
        ndt.close()


@pytest.mark.parametrize("att", list(GENERAL))
def test_point_scores_at_general_attitudes(pkg, O, att):
    """scorePoints: sums equal ndt_score_transform (rel 1e-12) for every neighbourhood, per-point values against the
    oracle with test_gpu_point_scores' sampler (every point within 1e-3 of a voxel face, and 512 drawn)."""
    s = scene("c1", att)
    ndt = engine(pkg, "c1")
    try:
        ndt.setInputSource(s["source"])
        for method in (pkg.DIRECT1, pkg.DIRECT7, pkg.DIRECT26, pkg.KDTREE):
            ndt.setParams(search_method=method)
            for T in (s["P"], s["aligned"]):
                check_sums(ndt, T)
    finally:
        ndt.close()
    per_point_case(pkg, O, s["source"], s["target"], s["P"], 1.0, 512)


@pytest.mark.parametrize("att", ["general-a", "general-c"])
def test_fitness_at_general_attitudes(pkg, att):
    """getFitnessScore against the brute-force f64 nearest distance of test_gpu_fitness, at the guess and aligned"""
    s = scene("c1", att)
    ndt = engine(pkg, "c1")
    try:
        ndt.setInputSource(s["source"])
        check_pose(ndt, s["target"], s["P"])
        T = ndt.align(s["P"])
        _, got = check_pose(ndt, s["target"], T)
        assert ndt.getFitnessScore() == got["fitness_score"]
    finally:
        ndt.close()


# ---------------------------------------------------------------------------------------- 3. align
@pytest.mark.parametrize("att", ALIGN)
@pytest.mark.parametrize("name", SCENES)
def test_align_from_every_attitude(pkg, O, S, name, att):
    """ndt_align(P') against the oracle: every evaluation of the oracle's f64 trajectory through the batched kernel and
    every evaluation the align itself made (single-pose kernel, pre-launched or not) against the oracle, as
    test_gpu_trajectory / test_gpu_launch_shapes do; the same iterations and evaluations; the final pose within
    1e-6 m of the f64 trajectory's and 1 mm / 0.1 mrad (plus the oracle's own f64 / f32 gap) of the reference arithmetic's."""
    s = scene(name, att)
    src, P = s["source"], s["P"]
    grid = oracle_grid(name)
    prm64 = O.default_params(num_threads=ORACLE_THREADS, pair_mode=2, **KW)
    prm32 = O.default_params(num_threads=ORACLE_THREADS, pair_mode=0, **KW)
    ndt = engine(pkg, name)
    try:
        ndt.setInputSource(src)
        r64, log64 = _oracle_trajectory(pkg, O, grid, src, P, pkg.default_params(**KW), prm64)
        worst = dict(score=0.0, g=0.0, g_abs=0.0, H=0.0)
        gmax = max(np.linalg.norm(e["d"]["gradient"]) for e in log64)
        for e in log64:
            got = ndt.evalDerivatives(e["pose"], transforms=[e["T"]], compute_hessian=e["need_h"])[0]
            d = e["d"]
            assert got["n_pairs"] == d["n_pairs"] and got["n_with_neighbors"] == d["n_with_neighbors"]
            worst["score"] = max(worst["score"], abs(got["score"] - d["score"]) / abs(d["score"]))
            worst["g"] = max(worst["g"], np.linalg.norm(got["gradient"] - d["gradient"]) /
                             max(np.linalg.norm(d["gradient"]), 1e-300))
            worst["g_abs"] = max(worst["g_abs"], np.linalg.norm(got["gradient"] - d["gradient"]) / gmax)
            if e["need_h"]:
                worst["H"] = max(worst["H"], np.linalg.norm(got["hessian"] - d["hessian"]) / np.linalg.norm(d["hessian"]))
        ndt.debugEvalLog(512)
        T = ndt.align(P)
        own = ndt.debugEvalLogRead()
        ndt.debugEvalLog(0)
        res = ndt.getResult()
        ref = grid.align(src, P, params=prm32)
        dt64, dr64 = S.pose_error(T, r64["T"])
        dt, dr = S.pose_error(T, ref["T"])
        print("ALIGN %-4s %-14s iterations %d / f64 %d / ref %d  replay score %.1e g %.1e (own %.1e) H %.1e  "
              "vs f64 %.1e m %.1e rad  vs ref %.1e m %.1e rad" % (name, att, res["iterations"], r64["iterations"],
              ref["iterations"], worst["score"], worst["g_abs"], worst["g"], worst["H"], dt64, dr64, dt, dr))
        assert worst["score"] < 1e-9 and worst["H"] < 1e-9 and worst["g_abs"] < 1e-9 and worst["g"] < 1e-6, worst
        # the align's own evaluations
        assert own and all(e["K"] == 1 and e["desc"]["batch"] == 0 for e in own)
        # the loop starts from the guess matrix itself and the Euler angles the host takes from it -- the folded triple
        # (roll + pi, pi - pitch, yaw + pi) where the first raw angle is positive
        assert np.array_equal(own[0]["T32"], np.asarray(P, np.float32).T.ravel())
        np.testing.assert_allclose(own[0]["pose6"], O.matrix_to_pose(P), atol=1e-12)
        for i, e in enumerate(own):
            ref_e = grid.derivatives(src, e["pose6"], T=e["T"], compute_hessian=e["need_h"], params=prm64)
            compare(words_of(pkg, e), ref_e, gmax, e["need_h"], (name, att, "own evaluation", i))
        assert res["converged"] and r64["converged"] and ref["converged"]
        assert res["iterations"] == r64["iterations"], (res["iterations"], r64["iterations"])
        assert res["n_evaluations"] == _distinct_poses(log64), (res["n_evaluations"], len(log64))
        assert dt64 < 1e-6 and dr64 < 1e-7, (dt64, dr64)
        np.testing.assert_allclose(res["hessian"], r64["hessian"], rtol=0, atol=1e-9 * np.abs(r64["hessian"]).max())
        # The reference's own arithmetic (f32 per-pair products): the oracle against itself, f64 products against f32, ends
        # 1e-8 .. 5e-4 m apart at most of these attitudes but 2.5 mm at roll pi - 1e-3 (C1) and 8 mm .. 0.19 m next to
        # the gimbal corner, where the Euler-angle Newton step is ill-conditioned and a last-bit difference moves a
        # line-search decision.  As in tests/test_gpu_parity.py::test_km_scale_coordinates the kernel, which carries f64,
        # is held to the f64 trajectory above and to the reference arithmetic at that gap plus the align bound.
        gap_t, gap_r = S.pose_error(r64["T"], ref["T"])
        print("      oracle f64 vs f32 products: %.1e m %.1e rad" % (gap_t, gap_r))
        assert dt < gap_t + ALIGN_TOL_M and dr < gap_r + ALIGN_TOL_RAD, (dt, dr, gap_t, gap_r)
        # the reference test's 0.05 m / 0.035 rad from the true pose, wherever the oracle's own align meets them (next to
        # the gimbal corner it stops 0.05 .. 0.07 m short)
        gt_t, gt_r = S.pose_error(T, s["aligned"])
        o_t, o_r = S.pose_error(r64["T"], s["aligned"])
        if o_t < 0.05 and o_r < 0.035:
            assert gt_t < 0.05 and gt_r < 0.035, (gt_t, gt_r)
    finally:
        ndt.close()


@pytest.mark.parametrize("name", SCENES)
def test_roll_pair_takes_both_branches_of_the_fold(pkg, O, S, name):
    """roll +0.3 and -0.3 at the same pitch and yaw: matrix_to_pose keeps the first and folds the second onto
    (roll + pi, pi - pitch, yaw + pi).  Each align ends within the align bound of the oracle's f64 one from the same guess
    (test_align_from_every_attitude holds each of them to all of its bounds)."""
    ndt = engine(pkg, name)
    try:
        ends = []
        for att, folded in (("roll+0.3", False), ("roll-0.3", True)):
            s = scene(name, att)
            p = O.matrix_to_pose(s["P"])
            r, pi_, y = ATTITUDES[att]
            want = np.array([r + PI, PI - pi_, y + PI]) if folded else np.array([r, pi_, y])
            assert np.abs(np.angle(np.exp(1j * (p[3:] - want)))).max() < 1e-6, (att, p, want)
            assert (abs(p[3]) > PI / 2) == folded
            ndt.setInputSource(s["source"])
            T = ndt.align(s["P"])
            ref = oracle_grid(name).align(s["source"], s["P"], params=O.default_params(num_threads=ORACLE_THREADS, pair_mode=2, **KW))
            dt, dr = S.pose_error(T, ref["T"])
            assert ndt.getResult()["converged"] and dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD, (att, dt, dr)
            ends.append(T @ np.linalg.inv(s["P"]))     # the correction the align found, in the map frame
        print("roll pair %s: corrections %.1e m %.1e rad apart" % ((name,) + S.pose_error(ends[0], ends[1])))
    finally:
        ndt.close()


# ---------------------------------------------------------------------------------------- 4. batch
def test_align_many_around_a_general_attitude(pkg, S):
    """Six guesses around P' (+-0.3 m, +-3 deg): each hypothesis of ndt_align_batch is ndt_align from that guess, bit
    for bit (tests/test_gpu_align_batch.py::test_c2_each_hypothesis_is_ndt_align)."""
    s = scene("c1", "general-b")
    ndt = engine(pkg, "c1")
    try:
        ndt.setInputSource(s["source"])
        g, d = s["P"], np.deg2rad(3.0)
        guesses = [g, g @ S.pose_matrix(0.3, 0.0, 0.0, 0.0, 0.0, d), g @ S.pose_matrix(-0.3, 0.0, 0.0, 0.0, 0.0, -d),
                   g @ S.pose_matrix(0.0, 0.3, 0.0, 0.0, 0.0, -d), s["aligned"], g @ S.pose_matrix(0.0, -0.3, 0.0, 0.0, 0.0, d)]
        serial = _serial(ndt, guesses)
        n0 = ndt.getTiming()["n_eval_launches"]
        got = ndt.alignMany(guesses)
        launched = ndt.getTiming()["n_eval_launches"] - n0
        assert len(got) == len(guesses)
        for k, ((T, r), one) in enumerate(zip(got, serial)):
            assert np.array_equal(T, one["T"]), k
            _assert_same(r, one, k)
        evals = [one["n_evaluations"] for one in serial]
        assert launched == max(evals) < sum(evals)
        assert sum(one["converged"] for one in serial) >= 3
    finally:
        ndt.close()


# ---------------------------------------------------------------------------------------- 5. SVN
@pytest.mark.parametrize("prior", ["near-the-cut", "general-a"])
def test_svn_at_large_attitudes(pkg, O, S, prior):
    """ndt_svn_align with the prior at (0.3, 1.2, pi - 1e-3) and at a general attitude, K = 4, five iterations: the
    particles follow the oracle's to the bound of tests/test_svn.py::test_hip_svn_matches_oracle."""
    s = scene_at("c1", (0.3, 1.2, PI - 1e-3), (0.2, -0.3, 0.4)) if prior == "near-the-cut" else scene("c1", prior)
    K, iters = 4, 5
    prm = O.default_params(resolution=1.0, min_points_per_voxel=3, hessian_mode=O.HESSIAN_GAUSS_NEWTON,
                           add_ridge=1, num_threads=8)
    grid = O.Grid(s["target"], prm)
    particles = pkg.svn_sample_particles(s["P"], K, seed=7)
    np.testing.assert_allclose(particles, O.svn_sample_particles(s["P"], K, 7), atol=1e-12)
    ref = O.svn_align(grid, s["source"], s["P"], particles, prm, max_iterations=iters, kernel_bandwidth=1.0,
                      step_size=1.0, stop_threshold=1e-4)
    svn = pkg.SvnNormalDistributionsTransform(device_id=0, resolution=1.0, min_points_per_voxel=3)
    try:
        svn.setParticleCount(K); svn.setMaxIterations(iters); svn.setKernelBandwidth(1.0)
        svn.setStepSize(1.0); svn.setEarlyStopThreshold(1e-4)
        svn.setNeighborhoodSearchMethod(pkg.DIRECT7)
        svn.setInputTarget(s["target"])
        got = svn.align(s["source"], s["P"], particles=particles)
    finally:
        svn.close()
    assert got["converged"] == ref["converged"]
    assert abs(got["iterations"] - ref["iterations"]) <= 2
    dt, dr = S.pose_error(got["final_pose"], ref["pose"])
    worst = [max(S.pose_error(a, b)[i] for a, b in zip(got["particles"], ref["particles"])) for i in (0, 1)]
    moved = max(S.pose_error(a, b)[0] for a, b in zip(got["particles"], particles))
    print("SVN %s: %d iterations, mean %.1e m %.1e rad from the oracle's, particles %.1e m %.1e rad (moved %.2f m)"
          % (prior, got["iterations"], dt, dr, worst[0], worst[1], moved))
    assert dt < 1e-3 and dr < 1e-4, (dt, dr)
    assert worst[0] < 2e-3 and worst[1] < 2e-4, worst
    assert moved > 1e-3          # the iteration did something
