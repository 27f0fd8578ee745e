"""Continuous-time NDT on the device (ndt_set_source_times / _device, ndt_eval_derivatives_ct, ndt_align_ct,
ndt_transform_source_ct / _device) against the NumPy restatement of the header's rule (test_ct_cpu.ct_numpy /
ct_apply_numpy), fed with the engine's own getLeaves() and getGridInfo().
Scene (test_ct_cpu.scene): hilly ground and building faces on 28 m x 28 m, 9 000 target points at a 1.0 m leaf; the source
is a scan of 4 500 points recorded while the sensor moves 0.6 m and turns 2 degrees, one time factor per point.
Tolerances are those of tests/test_gpu_d2d.py for "the same formulas in f64": score and nvtl_sum 1e-9 relative, gradient
and Hessian 1e-9 of their norms, the three counters equal; the align within 1 mm / 0.1 mrad of the CPU run of
ndt_newton_align over the restatement, its iteration count within one of it.
The transform's bit equality with NumPy rests on sin and cos of the point's angles being the same f64 on both sides or
one ulp apart: the result is rounded to f32 once, 29 bits further up, so an ulp shows in about one coordinate in 2^28."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_ct_cpu import (ALIGN_TOL_M, ALIGN_TOL_RAD, B_TRUE, E_RAW_MIN_M, E_RAW_MIN_RAD, P_TRUE, RIGID_POSE, GUESS_OFF,
                         assert_close_all_round, assert_close_to_f32_transform, ct_apply_numpy, ct_moved, ct_numpy, face_distance, newton_over_restatement,
                         rigid_source, scene)
from test_d2d_cpu import KW, gauss_constants
from test_gpu_d2d import assert_matches
from test_gpu_map_target import code_of

pytestmark = pytest.mark.gpu

INVALID_ARG, NO_TARGET, NO_SOURCE, UNSUPPORTED = -1, -4, -5, -9
SIZES = (1, 63, 64, 257, 1000, 4099)   # a partial wave, a full wave, one lane past a block, 17 blocks (> 8 sum segments, no multiple)
POSE = P_TRUE + GUESS_OFF


def engine(pkg, **kw):
    return pkg.NormalDistributionsTransform(device_id=0, resolution=1.0, **dict(KW, **kw))


@pytest.fixture(scope="module")
def rig(pkg):
    s = scene()
    A = engine(pkg)
    A.setInputTarget(s["target"])
    d1, d2 = gauss_constants(pkg)
    return dict(s, A=A, leaves=A.getLeaves(), grid=A.getGridInfo(), d1=d1, d2=d2)


def special_source(rig, n):
    """n points and times off the raw scan, with the cases of the rule among them as far as n has room: points outside
    the grid, points in cells without a leaf (above the scene), a NaN coordinate, a NaN and an infinite time, times of
    exactly 0 and 1, and times below 0 and above 1"""
    src, alpha = rig["raw"][:n].copy(), rig["alpha"][:n].copy()
    if n == 1:
        return src, alpha
    edits = [("alpha", 0.0), ("alpha", 1.0), ("alpha", -0.5), ("alpha", 1.5), ("alpha", np.nan), ("alpha", np.inf),
             ("alpha", -np.inf), ("x", np.nan), ("far", 500.0), ("far", -500.0), ("top", 2.5), ("top", 4.5)]
    at = np.linspace(1, n - 1, len(edits)).astype(int) if n > 2 * len(edits) else np.arange(1, min(n, len(edits) + 1))
    g = rig["grid"]
    for k, (what, val) in zip(at, edits):
        if what == "alpha":
            alpha[k] = val
        elif what == "x":
            src[k, 1] = val
        elif what == "far":
            src[k, 0] = val
        else:
            # the top layer of the grid, `val` cells in from its low corner: only the tallest wall reaches up there
            c = np.array([g["min_b"][0] + val, g["min_b"][1] + val, g["max_b"][2] + 0.5]) * g["leaf_size"]
            src[k] = (c - POSE[:3]).astype(np.float32)
    return src, alpha


def empty_cells_hit(rig, src, alpha):
    """points that land inside the grid in a cell without a leaf"""
    from test_d2d_cpu import classify
    m = ct_moved(B_TRUE, POSE, src, alpha)[2]
    cell = classify(m.astype(np.float32), rig["grid"])
    return int(((cell >= 0) & ~np.isin(cell, rig["leaves"]["cell"])).sum())


def set_scan(pkg, ndt, src, alpha):
    ndt.setInputSource(src)
    assert pkg.setSourceTimes(ndt, alpha) == len(src)


def words_of(pkg, ndt, begin, poses, hessian=True):
    return pkg.evalDerivativesCT(ndt, begin, poses, compute_hessian=hessian, raw=True).view(np.uint64).copy()


# ---- 1. the evaluation is the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("hessian", [True, False], ids=["hessian", "gradient"])
@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT1"])
def test_evaluation_equals_the_restatement(pkg, rig, method, hessian):
    A = rig["A"]
    A.setNeighborhoodSearchMethod(pkg.DIRECT7 if method == "DIRECT7" else pkg.DIRECT1)
    try:
        for n in SIZES:
            src, alpha = special_source(rig, n)
            # the precondition on the INPUTS, as in the D2D tests: no moved point within 1e-6 of a voxel face
            assert face_distance(ct_moved(B_TRUE, POSE, src, alpha)[2]) >= 1e-6, n
            set_scan(pkg, A, src, alpha)
            want = ct_numpy(B_TRUE, POSE, src, alpha, rig["leaves"], rig["grid"], rig["d1"], rig["d2"], method, hessian=hessian)
            got = pkg.evalDerivativesCT(A, B_TRUE, POSE, compute_hessian=hessian)[0]
            assert_matches(got, want)
            if not hessian:
                assert not got["hessian"].any()
            if n == SIZES[-1]:
                assert want["n_pairs"] > (5000 if method == "DIRECT7" else 1500)
                assert want["n_with_neighbors"] < n - 8                       # the special points found nothing
                assert empty_cells_hit(rig, src, alpha) >= 2
                print("%s: %d points, %d pairs, score %.6f" % (method, n, want["n_pairs"], want["score"]))
            if n >= 64:
                # times below 0 and above 1 are the times 0 and 1, bit for bit
                clamped = np.where(np.isfinite(alpha), np.clip(alpha, 0.0, 1.0), alpha).astype(np.float32)
                assert (clamped != alpha)[np.isfinite(alpha)].sum() == 2
                w = words_of(pkg, A, B_TRUE, POSE, hessian)
                assert pkg.setSourceTimes(A, clamped) == n
                assert np.array_equal(words_of(pkg, A, B_TRUE, POSE, hessian), w)
    finally:
        A.setNeighborhoodSearchMethod(pkg.DIRECT7)


# ---- 2. every alpha = 1: the engine's own evaluation --------------------------------------------------------------------
@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT1"])
def test_alpha_one_is_the_rigid_evaluation(pkg, rig, method):
    """ndt_eval_derivatives moves the points with an f32 matrix, the CT evaluation in f64: 1e-6 all round, at the pose
    whose f32 matrix is exact (the reasons stand in test_ct_cpu.test_alpha_one_is_the_oracles_evaluation)."""
    A = rig["A"]
    A.setNeighborhoodSearchMethod(pkg.DIRECT7 if method == "DIRECT7" else pkg.DIRECT1)
    try:
        src = rigid_source(rig)
        ones = np.ones(len(src), np.float32)
        assert face_distance(ct_moved(B_TRUE, RIGID_POSE, src, ones)[2]) >= 1e-6
        set_scan(pkg, A, src, ones)
        want = A.evalDerivatives(RIGID_POSE)[0]
        got = pkg.evalDerivativesCT(A, B_TRUE, RIGID_POSE)[0]
        assert want["n_pairs"] > 1000
        assert_close_all_round(got, want, 1e-6)
    finally:
        A.setNeighborhoodSearchMethod(pkg.DIRECT7)


@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT1"])
def test_alpha_one_at_a_vehicle_attitude_is_the_rigid_evaluation(pkg, rig, method):
    """the same comparison at the scan's own attitude, where the engine's f32 matrix is the f64 rotation slightly turned:
    to the bound test_ct_cpu derives from that (assert_close_to_f32_transform)"""
    A = rig["A"]
    A.setNeighborhoodSearchMethod(pkg.DIRECT7 if method == "DIRECT7" else pkg.DIRECT1)
    try:
        set_scan(pkg, A, rig["ideal"], np.ones(len(rig["ideal"]), np.float32))
        want = A.evalDerivatives(POSE)[0]
        got = pkg.evalDerivativesCT(A, B_TRUE, POSE)[0]
        assert want["n_pairs"] > 1000
        assert_close_to_f32_transform(got, want)
    finally:
        A.setNeighborhoodSearchMethod(pkg.DIRECT7)


# ---- 2b. the begin pose on another Euler branch than the end pose ---------------------------------------------------------
def other_triple(p):
    """the other Euler triple of the same rotation"""
    return np.array([p[0], p[1], p[2], p[3] + np.pi, np.pi - p[4], p[5] + np.pi])


def test_begin_pose_is_fitted_to_the_end_poses_branch(pkg, rig):
    """Results of consecutive aligns lie on different Euler triples whenever the roll changes sign, and on different turns
    when the yaw crosses pi: evaluation and deskew fit the begin pose to the end pose as the align does.  The same scan
    under the same two rotations written four ways gives the restatement's numbers (which fits by the header's rule), the
    score of the plain writing to rounding, and the ideally deskewed scan."""
    A = rig["A"]
    src, alpha = rig["raw"], rig["alpha"]
    set_scan(pkg, A, src, alpha)
    args = (rig["leaves"], rig["grid"], rig["d1"], rig["d2"])
    plain = pkg.evalDerivativesCT(A, B_TRUE, P_TRUE)[0]
    turn = np.array([0, 0, 0, 0, 0, 2 * np.pi])
    ways = {"end on the other triple": (B_TRUE, other_triple(P_TRUE)), "begin on the other triple": (other_triple(B_TRUE), P_TRUE),
            "begin a turn ahead": (B_TRUE + turn, P_TRUE), "end a turn behind, on the other triple": (B_TRUE, other_triple(P_TRUE) - turn)}
    for name, (b, e) in ways.items():
        got = pkg.evalDerivativesCT(A, b, e)[0]
        assert_matches(got, ct_numpy(b, e, src, alpha, *args))
        assert got["n_pairs"] == plain["n_pairs"] and got["score"] == pytest.approx(plain["score"], rel=1e-9), name
        for frame in (0, 1):
            y = pkg.transformSourceCT(A, b, e, frame)
            assert np.array_equal(bits(y), bits(ct_apply_numpy(b, e, src, alpha, frame))), (name, frame)
        y = pkg.transformSourceCT(A, b, e, 0)
        assert np.abs(y.astype(np.float64) - rig["ideal"]).max() < 8 * np.spacing(np.float32(16.0)), name
    # a yaw that crosses pi within the scan: the whole scene turned by c about z (Rz is the innermost rotation, so the raw
    # scan turned by -c under poses whose yaws are c further on is the same scan); the end pose's yaw comes back wrapped
    c = np.pi - 0.02
    from slam_sam_amd import synth
    back = synth.pose_matrix(0, 0, 0, 0, 0, -c)
    b, e = B_TRUE + [0, 0, 0, 0, 0, c], P_TRUE + [0, 0, 0, 0, 0, c - 2 * np.pi]
    assert b[5] > 3.1 and e[5] < -3.1
    turned = synth.transform(back, src).astype(np.float32)
    set_scan(pkg, A, turned, alpha)
    y = pkg.transformSourceCT(A, b, e, 0)
    assert np.array_equal(bits(y), bits(ct_apply_numpy(b, e, turned, alpha, 0)))
    want = synth.transform(back, rig["ideal"])
    assert np.abs(y.astype(np.float64) - want).max() < 8 * np.spacing(np.float32(16.0))


# ---- 3. b == p ------------------------------------------------------------------------------------------------------------
def test_equal_poses_do_not_see_the_times(pkg, rig):
    """b == p: the points land where the rigid evaluation puts them whatever their times are -- score, nvtl_sum and the
    counters are bit-equal under shuffled times.  Gradient and Hessian carry a_i and a_i^2 by the rule (the derivative
    with respect to the end pose; test_ct_cpu.test_equal_poses_do_not_see_the_times): they equal the restatement's."""
    A = rig["A"]
    src, alpha = rig["raw"], rig["alpha"]
    shuffled = np.random.default_rng(4).permutation(alpha)
    set_scan(pkg, A, src, alpha)
    w0 = words_of(pkg, A, POSE, POSE)
    g0 = pkg.evalDerivativesCT(A, POSE, POSE)[0]
    assert pkg.setSourceTimes(A, shuffled) == len(src)
    w1 = words_of(pkg, A, POSE, POSE)
    g1 = pkg.evalDerivativesCT(A, POSE, POSE)[0]
    assert g0["n_pairs"] > 5000
    assert np.array_equal(w0[0, [0, 28, 29, 30, 31]], w1[0, [0, 28, 29, 30, 31]])
    assert_matches(g0, ct_numpy(POSE, POSE, src, alpha, rig["leaves"], rig["grid"], rig["d1"], rig["d2"]))
    assert_matches(g1, ct_numpy(POSE, POSE, src, shuffled, rig["leaves"], rig["grid"], rig["d1"], rig["d2"]))
    # one common factor 0.5: the gradient halves and the Hessian quarters bit for bit, the ones of alpha = 1
    assert pkg.setSourceTimes(A, np.ones(len(src), np.float32)) == len(src)
    one = pkg.evalDerivativesCT(A, POSE, POSE)[0]
    assert pkg.setSourceTimes(A, np.full(len(src), 0.5, np.float32)) == len(src)
    half = pkg.evalDerivativesCT(A, POSE, POSE)[0]
    assert half["score"] == one["score"]
    assert np.array_equal(half["gradient"], 0.5 * one["gradient"]) and np.array_equal(half["hessian"], 0.25 * one["hessian"])


# ---- 4. bits --------------------------------------------------------------------------------------------------------------
def test_bit_identity(pkg, rig):
    A = rig["A"]
    set_scan(pkg, A, *special_source(rig, 4099))
    poses = np.stack([POSE, P_TRUE, POSE + [0.1, 0.05, -0.02, 0.004, 0.003, -0.01]])
    w3 = words_of(pkg, A, B_TRUE, poses)
    assert np.array_equal(w3, words_of(pkg, A, B_TRUE, poses))                       # two calls
    for k in range(3):                                                               # a pose alone = the pose in a batch
        assert np.array_equal(words_of(pkg, A, B_TRUE, poses[k])[0], w3[k]), k
    assert len({w.tobytes() for w in w3}) == 3
    # without the Hessian: its words are zero, score / gradient / counters are the SAME BITS
    w0 = words_of(pkg, A, B_TRUE, poses, hessian=False)
    assert not w0[:, 7:28].any() and w3[:, 7:28].any()
    assert np.array_equal(w0[:, :7], w3[:, :7]) and np.array_equal(w0[:, 28:], w3[:, 28:])


# ---- 5. the times' life cycle -----------------------------------------------------------------------------------------------
def test_times_lifecycle(pkg, rig, hipmem):
    A = engine(pkg)
    A.setInputTarget(rig["target"])
    src, alpha = rig["raw"][:1000], rig["alpha"][:1000]
    L = pkg.lib()
    assert pkg.sourceTimesInfo(A) == 0
    assert code_of(pkg, pkg.evalDerivativesCT, A, B_TRUE, POSE) == NO_SOURCE        # no source at all
    A.setInputSource(src)
    assert code_of(pkg, pkg.evalDerivativesCT, A, B_TRUE, POSE) == NO_SOURCE        # a source without times
    assert "times" in L.ndt_last_error(A._h).decode()
    assert code_of(pkg, pkg.transformSourceCT, A, B_TRUE, POSE) == NO_SOURCE
    assert code_of(pkg, pkg.alignContinuousTime, A, B_TRUE) == NO_SOURCE
    assert pkg.setSourceTimes(A, alpha) == 1000
    before = words_of(pkg, A, B_TRUE, POSE)
    # a wrong n is refused and the old times still serve
    assert code_of(pkg, pkg.setSourceTimes, A, alpha[:999]) == INVALID_ARG
    assert code_of(pkg, pkg.setSourceTimes, A, np.zeros(1001, np.float32)) == INVALID_ARG
    d_alpha = hipmem.upload(alpha)
    assert code_of(pkg, pkg.setSourceTimesDevice, A, d_alpha, 999) == INVALID_ARG
    assert pkg.sourceTimesInfo(A) == 1000 and np.array_equal(words_of(pkg, A, B_TRUE, POSE), before)
    # no existing call notices the times
    ev = A.evalDerivatives(POSE)[0]
    assert pkg.setSourceTimes(A, np.zeros(0, np.float32)) == 0                       # n == 0 clears
    assert code_of(pkg, pkg.evalDerivativesCT, A, B_TRUE, POSE) == NO_SOURCE
    ev2 = A.evalDerivatives(POSE)[0]
    assert ev["score"] == ev2["score"] and np.array_equal(ev["gradient"], ev2["gradient"])
    # the device setter gives the bits of the host setter
    assert pkg.setSourceTimesDevice(A, d_alpha, 1000) == 1000
    assert np.array_equal(words_of(pkg, A, B_TRUE, POSE), before)
    # every call that replaces or re-declares the source drops the times
    dx, dy, dz = (hipmem.upload(np.ascontiguousarray(src[:, k])) for k in range(3))
    A.putKeyframe(7, src)
    setters = {
        "setInputSource": lambda: A.setInputSource(src),
        "setInputSourceSoA": lambda: A.setInputSourceSoA(src[:, 0].copy(), src[:, 1].copy(), src[:, 2].copy()),
        "setInputSourceDevice": lambda: A.setInputSourceDevice(dx, dy, dz, 1000),
        "setInputSourceDeviceView": lambda: A.setInputSourceDeviceView(dx, dy, dz, 1000),
        "sourceChanged": lambda: A.sourceChanged(),
        "setInputSourceFromKeyframe": lambda: A.setInputSourceFromKeyframe(7),
    }
    for name, call in setters.items():
        assert pkg.setSourceTimes(A, alpha) == 1000, name
        assert np.array_equal(words_of(pkg, A, B_TRUE, POSE), before), name          # the same points every time
        call()
        assert pkg.sourceTimesInfo(A) == 0, name
        assert code_of(pkg, pkg.evalDerivativesCT, A, B_TRUE, POSE) == NO_SOURCE, name
        assert code_of(pkg, pkg.transformSourceCT, A, B_TRUE, POSE) == NO_SOURCE, name


# ---- 6. unsupported configurations, missing target ------------------------------------------------------------------------
def test_unsupported_configurations(pkg, rig):
    A = rig["A"]
    set_scan(pkg, A, rig["raw"], rig["alpha"])
    before = words_of(pkg, A, B_TRUE, POSE)
    try:
        for method in (pkg.KDTREE, pkg.DIRECT26):
            A.setNeighborhoodSearchMethod(method)
            assert code_of(pkg, pkg.evalDerivativesCT, A, B_TRUE, POSE) == UNSUPPORTED
            assert code_of(pkg, pkg.alignContinuousTime, A, B_TRUE) == UNSUPPORTED
    finally:
        A.setNeighborhoodSearchMethod(pkg.DIRECT7)
    assert np.array_equal(words_of(pkg, A, B_TRUE, POSE), before)
    U = engine(pkg)                                                                  # a multi-grid union target
    U.addTarget(rig["target"][:4500], 0)
    U.addTarget(rig["target"][4500:], 1)
    U.createVoxelKdtree()
    set_scan(pkg, U, rig["raw"], rig["alpha"])
    assert code_of(pkg, pkg.evalDerivativesCT, U, B_TRUE, POSE) == UNSUPPORTED
    H = engine(pkg)                                                                  # a hook reducer
    H.setInputTarget(rig["target"])
    set_scan(pkg, H, rig["raw"], rig["alpha"])
    assert pkg.evalDerivativesCT(H, B_TRUE, POSE)[0]["n_pairs"] > 0
    H.commInitHook(lambda _ctx, _w, _n: 0, 0, 1)
    assert code_of(pkg, pkg.evalDerivativesCT, H, B_TRUE, POSE) == UNSUPPORTED
    assert code_of(pkg, pkg.alignContinuousTime, H, B_TRUE) == UNSUPPORTED
    # no target: the guess comes back
    N = engine(pkg)
    set_scan(pkg, N, rig["raw"], rig["alpha"])
    assert code_of(pkg, pkg.evalDerivativesCT, N, B_TRUE, POSE) == NO_TARGET
    res = pkg.Result()
    g = np.ascontiguousarray(np.eye(4, dtype=np.float32).T).ravel()
    g[12] = 0.5
    b = np.ascontiguousarray(B_TRUE)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    assert pkg.lib().ndt_align_ct(N._h, b.ctypes.data_as(dp), g.ctypes.data_as(fp), C.byref(res)) == NO_TARGET
    assert res.converged == 0 and list(res.final_transformation) == list(g)
    N.setInputTarget(rig["target"])
    N.setInputSource(rig["raw"])                                                     # ... and without times
    assert pkg.lib().ndt_align_ct(N._h, b.ctypes.data_as(dp), g.ctypes.data_as(fp), C.byref(res)) == NO_SOURCE
    assert res.converged == 0 and list(res.final_transformation) == list(g)


# ---- 7. the align ---------------------------------------------------------------------------------------------------------
def test_align_follows_newton_over_the_restatement(pkg, rig):
    """Measured on an MI355X: 5 iterations (the restatement 5), 1.1e-16 m / 2.3e-18 rad from it; e_rigid 0.00147 m /
    3.07e-4 rad, e_raw 0.23397 m / 1.79e-2 rad, e_ct 0.00307 m / 3.51e-4 rad."""
    from slam_sam_amd import synth
    A = rig["A"]
    guess, truth = rig["guess"], rig["truth"]
    A.setInputSource(rig["ideal"])
    e_rigid = synth.pose_error(A.align(guess), truth)
    set_scan(pkg, A, rig["raw"], rig["alpha"])
    T0 = A.align(guess)                                                              # the rigid align of the raw scan
    r0, h0 = A.getResult(), A.getIterationHistory()
    e_raw = synth.pose_error(T0, truth)
    T, r = pkg.alignContinuousTime(A, B_TRUE, guess)
    ref = newton_over_restatement(pkg, rig)
    dt, dr = synth.pose_error(T, ref["T"])
    e_ct = synth.pose_error(T, truth)
    print("alignContinuousTime: %d iterations (restatement %d), %.2e m %.2e rad from it" % (r["iterations"], ref["iterations"], dt, dr))
    print("e_rigid %.5f m %.2e rad, e_raw %.5f m %.2e rad, e_ct %.5f m %.2e rad" % (e_rigid + e_raw + e_ct))
    assert r["converged"] and ref["converged"]
    assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD
    assert abs(r["iterations"] - ref["iterations"]) <= 1
    assert e_raw[0] >= E_RAW_MIN_M and e_raw[1] >= E_RAW_MIN_RAD
    assert e_ct[0] <= 4.0 * e_rigid[0] + ALIGN_TOL_M and e_ct[1] <= 4.0 * e_rigid[1] + ALIGN_TOL_RAD
    # a begin pose a whole turn away is brought onto the guess's branch
    T2, r2 = pkg.alignContinuousTime(A, B_TRUE + [0, 0, 0, 0, 0, 2 * np.pi], guess)
    assert r2["iterations"] == r["iterations"] and synth.pose_error(T2, T)[0] < 1e-6
    # a guess with a slightly negative roll: the engine's matrix-to-pose conversion puts it on the other Euler triple (roll
    # near pi), and the begin pose is brought there with it
    T3, r3 = pkg.alignContinuousTime(A, B_TRUE, synth.pose_matrix(*(P_TRUE + GUESS_OFF + [0, 0, 0, -2 * P_TRUE[3], 0, 0])))
    e3 = synth.pose_error(T3, truth)
    print("from a guess with a negative roll: pose %s, %.5f m %.2e rad from the true end pose" % (np.round(r3["pose"], 4), e3[0], e3[1]))
    assert r3["converged"] and r3["pose"][3] > 3.0
    assert e3[0] <= 4.0 * e_rigid[0] + ALIGN_TOL_M and e3[1] <= 4.0 * e_rigid[1] + ALIGN_TOL_RAD
    # ... and the deskew under that result, begin and end on different triples, is the ideal scan up to the pose error
    # seen from at most 20 m (without the fit the blend would run the roll from 0 to pi: metres)
    y3 = pkg.transformSourceCT(A, B_TRUE, r3["pose"], 0)
    assert np.abs(y3.astype(np.float64) - rig["ideal"]).max() <= e3[0] + 20.0 * e3[1] + 1e-5
    # the handle's own align is left alone: history unchanged, the same bits again
    h1 = A.getIterationHistory()
    assert all(np.array_equal(a, b) for a, b in zip(h0, h1)) and len(h0[1]) > 1
    T1 = A.align(guess)
    r1 = A.getResult()
    assert np.array_equal(T1.view(np.uint64), T0.view(np.uint64))
    for k in ("pose", "hessian"):
        assert np.array_equal(np.asarray(r1[k]).view(np.uint64), np.asarray(r0[k]).view(np.uint64)), k
    assert (r1["iterations"], r1["n_evaluations"], r1["transform_probability"], r1["nvtl"]) == \
           (r0["iterations"], r0["n_evaluations"], r0["transform_probability"], r0["nvtl"])
    assert all(np.array_equal(a, b) for a, b in zip(h0, A.getIterationHistory()))


# ---- 8. the deskewed scan -------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_transform_source_ct(pkg, rig, hipmem):
    A = rig["A"]
    src, alpha = special_source(rig, 4099)
    set_scan(pkg, A, src, alpha)
    n = len(src)
    bad = ~(np.isfinite(src).all(axis=1) & np.isfinite(alpha))
    assert bad.sum() == 4
    for frame in (0, 1):
        got = pkg.transformSourceCT(A, B_TRUE, P_TRUE, frame)
        want = ct_apply_numpy(B_TRUE, P_TRUE, src, alpha, frame)
        assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()             # NaN rows where stated
        assert np.array_equal(bits(got)[~bad], bits(want)[~bad]), frame              # the restatement, bit for bit
        # the device form gives the same bits
        d = [hipmem.upload(np.full(n + 3, -7.0, np.float32)) for _ in range(3)]
        pkg.transformSourceCTDevice(A, B_TRUE, P_TRUE, d[0], d[1], d[2], n + 3, frame)
        back = np.zeros((3, n + 3), np.float32)
        for k in range(3):
            assert hipmem.rt.hipMemcpy(back[k].ctypes.data, C.c_void_p(d[k]), back[k].nbytes, 2) == 0
        assert np.array_equal(bits(back[:, :n].T), bits(got)) and np.all(back[:, n:] == -7.0)
    # the two exact cases of frame 0
    got = pkg.transformSourceCT(A, B_TRUE, P_TRUE, 0)
    ones = (np.clip(alpha, 0, 1) == 1.0) & ~bad
    assert ones.sum() == 2 and np.array_equal(bits(got)[ones], bits(src)[ones])      # a_i == 1
    same = pkg.transformSourceCT(A, P_TRUE, P_TRUE, 0)                               # b == e
    assert np.array_equal(bits(same)[~bad], bits(src)[~bad]) and np.isnan(same[bad]).all()
    # cap < n writes nothing
    out = np.full((n, 3), -7.0, np.float32)
    b, e = np.ascontiguousarray(B_TRUE), np.ascontiguousarray(P_TRUE)
    dp = C.POINTER(C.c_double)
    assert pkg.lib().ndt_transform_source_ct(A._h, b.ctypes.data_as(dp), e.ctypes.data_as(dp), 0, out.ctypes.data, n - 1) == INVALID_ARG
    assert np.all(out == -7.0)
    d = [hipmem.upload(np.full(n, -7.0, np.float32)) for _ in range(3)]
    assert code_of(pkg, pkg.transformSourceCTDevice, A, B_TRUE, P_TRUE, d[0], d[1], d[2], n - 1, 0) == INVALID_ARG
    chk = np.zeros(n, np.float32)
    assert hipmem.rt.hipMemcpy(chk.ctypes.data, C.c_void_p(d[0]), chk.nbytes, 2) == 0 and np.all(chk == -7.0)
    # at the true poses frame 0 is the ideally deskewed scan to within f32 rounding of the coordinates
    set_scan(pkg, A, rig["raw"], rig["alpha"])
    y = pkg.transformSourceCT(A, B_TRUE, P_TRUE, 0)
    assert np.abs(y.astype(np.float64) - rig["ideal"]).max() < 8 * np.spacing(np.float32(16.0))


# ---- 9. the C++ adapter ---------------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, rig, tmp_path):
    """tests/cpp/test_ct.cpp against the API mocks, built with the g++ line tests/cpp/Makefile uses for them; it reads the
    scene from a file this test writes and prints the end pose it found, which must be the Python call's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "tests", "cpp")
    exe = str(tmp_path / "test_ct")
    lib = os.path.join(root, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(root, "include", "compat"), "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(d, "test_ct.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    blob = str(tmp_path / "scene.bin")
    with open(blob, "wb") as f:
        np.array([len(rig["target"]), len(rig["raw"])], np.int64).tofile(f)
        np.concatenate([B_TRUE, rig["guess"].T.ravel()]).astype(np.float64).tofile(f)   # begin pose, guess column-major
        rig["target"].astype(np.float32).tofile(f)
        rig["raw"].astype(np.float32).tofile(f)
        rig["alpha"].astype(np.float32).tofile(f)
    p = subprocess.run([exe, blob], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ct: PASS" in p.stdout
    A = rig["A"]
    set_scan(pkg, A, rig["raw"], rig["alpha"])
    T, r = pkg.alignContinuousTime(A, B_TRUE, rig["guess"])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("end_pose ")][0]
    pose = np.array([float.fromhex(w) for w in line.split()[1:]])
    assert np.array_equal(pose, np.asarray(r["pose"]))                                # the same engine, the same bits
    y = pkg.transformSourceCT(A, B_TRUE, r["pose"], 0)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("deskewed_sum ")][0]
    assert float.fromhex(line.split()[1]) == float(np.cumsum(y.astype(np.float64).ravel())[-1])   # added in the same order
