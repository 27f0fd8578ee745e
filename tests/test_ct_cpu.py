"""CPU checks of the continuous-time registration (ndt_set_source_times / _device, ndt_source_times_info,
ndt_eval_derivatives_ct, ndt_align_ct, ndt_transform_source_ct / _device; no GPU): the seven symbols are declared,
exported, listed and bound with ABI version 3 unchanged; arguments are refused before the handle is looked at, and the
Python functions refuse misshapen input before the library is called; the kernels of ndt_ct.hip compile for gfx950 without
scratch.
The NumPy yardstick the GPU tests compare with lives here: `ct_numpy` is the evaluation rule of include/ndt_hip.h in f64
-- the point's pose, the moved point rotation after rotation as the header writes it, the pairs of test_d2d_cpu.d2d_pairs,
and per pair the rule's g_c and H_cd with j_c and h_cd taken from the DERIVATIVE MATRICES of Rx Ry Rz (not from the
kernel's chain) -- and `ct_apply_numpy` the rule of ndt_transform_source_ct.  Its own checks: gradient and Hessian against
central differences, alpha = 1 against the oracle, b == p independent of the times, the host Newton loop
(ndt_newton_align) driven by it on a scan captured in motion, and the usefulness condition: a rigid align of that scan
is biased, the continuous-time align is not."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from test_d2d_cpu import ATTITUDE, FD_STEP, FD_TOL, KW, d2d_pairs, gauss_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_set_source_times", "ndt_set_source_times_device", "ndt_source_times_info", "ndt_eval_derivatives_ct",
       "ndt_align_ct", "ndt_transform_source_ct", "ndt_transform_source_ct_device")
ALIGN_TOL_M, ALIGN_TOL_RAD = 1e-3, 1e-4                                      # the project's align tolerances
VEHICLE = (0.02, -0.03, 0.6)                                                  # a vehicle's attitude: nearly level, some heading


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def ct_fit_begin(begin, pose):
    """THE FIT of the header: the begin pose's angles on the Euler branch of the end pose's"""
    b, ref = np.asarray(begin, np.float64), np.asarray(pose, np.float64)[3:]
    cands = [np.array([b[3], b[4], b[5]]), np.array([b[3] + np.pi, np.pi - b[4], b[5] + np.pi])]
    dist = []
    for c in cands:
        for k in range(3):
            turns = np.floor(np.abs((c[k] - ref[k]) / (2.0 * np.pi)) + 0.5) * np.sign(c[k] - ref[k])   # round half away from zero
            if turns != 0.0:
                c[k] -= (2.0 * np.pi) * turns
        dist.append((np.abs(c[0] - ref[0]) + np.abs(c[1] - ref[1])) + np.abs(c[2] - ref[2]))
    return np.concatenate([b[:3], cands[1] if dist[1] < dist[0] else cands[0]])


def ct_point_poses(begin, pose, alpha):
    """(a [n], p_i [n, 6], counted [n]): the clamped factor, the point's pose and whether its time is finite"""
    b, p = ct_fit_begin(begin, pose), np.asarray(pose, np.float64)
    al = np.asarray(alpha, np.float32)
    ok = np.isfinite(al)
    a = np.clip(np.where(ok, al, np.float32(0)), np.float32(0), np.float32(1)).astype(np.float64)
    q = b[None, :] + a[:, None] * (p - b)[None, :]
    q = np.where((a == 1.0)[:, None], p[None, :], np.where((a == 0.0)[:, None], b[None, :], q))
    return a, q, ok


def ct_move(q, x):
    """x' of the header: u = Rz x, v = Ry u, w = Rx v, x' = w + t, every operation one f64 rounding"""
    x = np.asarray(x, np.float64)
    sr, cr, sp, cp, sy, cy = np.sin(q[:, 3]), np.cos(q[:, 3]), np.sin(q[:, 4]), np.cos(q[:, 4]), np.sin(q[:, 5]), np.cos(q[:, 5])
    u0, u1, u2 = cy * x[:, 0] - sy * x[:, 1], sy * x[:, 0] + cy * x[:, 1], x[:, 2]
    v0, v1, v2 = cp * u0 + sp * u2, u1, cp * u2 - sp * u0
    w0, w1, w2 = v0, cr * v1 - sr * v2, sr * v1 + cr * v2
    return np.stack([w0 + q[:, 0], w1 + q[:, 1], w2 + q[:, 2]], axis=1)


def rot_derivs_many(q):
    """R = Rx Ry Rz [n, 3, 3], dR [3][n, 3, 3] and d2R [3][3][n, 3, 3] of the angles of q [n, 6]"""
    n = len(q)
    zero, one = np.zeros(n), np.ones(n)

    def axis(a, k, which):
        c, s = np.cos(a), np.sin(a)
        cc, ss = ((c, s), (-s, c), (-c, -s))[k]
        o = one if k == 0 else zero
        rows = {"x": [[o, zero, zero], [zero, cc, -ss], [zero, ss, cc]],
                "y": [[cc, zero, ss], [zero, o, zero], [-ss, zero, cc]],
                "z": [[cc, -ss, zero], [ss, cc, zero], [zero, zero, o]]}[which]
        return np.stack([np.stack(r, axis=1) for r in rows], axis=1)

    def prod(o):
        return axis(q[:, 3], o[0], "x") @ axis(q[:, 4], o[1], "y") @ axis(q[:, 5], o[2], "z")

    unit = np.eye(3, dtype=int)
    return (prod((0, 0, 0)), [prod(tuple(unit[c])) for c in range(3)],
            [[prod(tuple(unit[c] + unit[d])) for d in range(3)] for c in range(3)])


def ct_moved(begin, pose, src, alpha):
    """(a, p_i, x' with NaN rows for the points that are not counted)"""
    a, q, ok = ct_point_poses(begin, pose, alpha)
    x = np.asarray(src, np.float32).astype(np.float64)
    ok = ok & np.isfinite(x).all(axis=1)
    with np.errstate(all="ignore"):
        m = ct_move(q, x)
    m[~ok] = np.nan
    return a, q, m


def sym_icov(leaves):
    """B: the triangle xx, xy, xz, yy, yz, zz of the leaves' icov, mirrored"""
    ic = np.asarray(leaves["icov"], np.float64)
    return ic[:, [0, 0, 0, 0, 1, 1, 0, 1, 2], [0, 1, 2, 1, 1, 2, 2, 2, 2]].reshape(-1, 3, 3)


def ct_numpy(begin, pose, src, alpha, leaves, grid, d1, d2, method="DIRECT7", hessian=True, pairs=None):
    """The evaluation rule: dict(score, gradient [6], hessian [6, 6], nvtl_sum, n_with_neighbors, n_pairs).
    src [n, 3] float32, alpha [n] float32; leaves: dict(cell [L] ascending, mean, icov) -- getLeaves();
    grid: dict(min_b, max_b, div_b, leaf_size) -- getGridInfo().  pairs: a fixed pair list (central differences)."""
    a, q, m = ct_moved(begin, pose, src, alpha)
    n = len(a)
    pi, ps = d2d_pairs(m, leaves, grid, method) if pairs is None else pairs
    out = dict(score=0.0, gradient=np.zeros(6), hessian=np.zeros((6, 6)), nvtl_sum=0.0, n_with_neighbors=0, n_pairs=0)
    if len(pi) == 0:
        return out
    mu = m[pi] - np.asarray(leaves["mean"], np.float64)[ps]
    B = sym_icov(leaves)[ps]
    v = np.einsum("pab,pb->pa", B, mu)
    with np.errstate(all="ignore"):
        e = np.exp(-d2 * np.einsum("pa,pa->p", mu, v) / 2.0)
    ok = np.isfinite(e) & (e >= 0.0) & (e <= 1.0)                          # the evaluation's guard
    pi, B, v, e = pi[ok], B[ok], v[ok], e[ok]
    P = len(pi)
    sc = -d1 * e
    best = np.zeros(n)
    np.maximum.at(best, pi, sc)
    out.update(score=float(sc.sum()), nvtl_sum=float(best.sum()), n_with_neighbors=len(np.unique(pi)), n_pairs=P)
    x = np.asarray(src, np.float32).astype(np.float64)[pi]
    _, dR, d2R = rot_derivs_many(q[pi])
    j = np.zeros((P, 6, 3))
    j[:, :3] = np.eye(3)
    for c in range(3):
        j[:, 3 + c] = np.einsum("pab,pb->pa", dR[c], x)
    vj = np.einsum("pa,pka->pk", v, j)                                       # mu^T B j_c
    f = d1 * d2 * e
    ap = a[pi]
    out["gradient"] = (ap[:, None] * f[:, None] * vj).sum(axis=0)
    if not hessian:
        return out
    t = -d2 * vj[:, :, None] * vj[:, None, :] + np.einsum("pda,pab,pcb->pcd", j, B, j)
    for c in range(3):
        for d in range(3):
            t[:, 3 + c, 3 + d] += np.einsum("pa,pa->p", v, np.einsum("pab,pb->pa", d2R[c][d], x))
    out["hessian"] = ((ap * ap * f)[:, None, None] * t).sum(axis=0)
    return out


def ct_apply_numpy(begin, end, src, alpha, frame=0):
    """ndt_transform_source_ct's rule: [n, 3] float32"""
    e = np.asarray(end, np.float64)
    a, q, m = ct_moved(begin, end, src, alpha)
    y = m
    if frame == 0:
        sr, cr, sp, cp, sy, cy = np.sin(e[3]), np.cos(e[3]), np.sin(e[4]), np.cos(e[4]), np.sin(e[5]), np.cos(e[5])
        w0, w1, w2 = m[:, 0] - e[0], m[:, 1] - e[1], m[:, 2] - e[2]
        v0, v1, v2 = w0, cr * w1 + sr * w2, cr * w2 - sr * w1
        u0, u1, u2 = cp * v0 - sp * v2, v1, sp * v0 + cp * v2
        y = np.stack([cy * u0 + sy * u1, cy * u1 - sy * u0, u2], axis=1)
    with np.errstate(all="ignore"):
        out = y.astype(np.float32)
    if frame == 0:
        same = np.isfinite(m).all(axis=1) & (q == e[None, :]).all(axis=1)
        out[same] = np.asarray(src, np.float32)[same]
    return out


# ---- the scene ----------------------------------------------------------------------------------------------------------
# A scan captured in motion: the sensor goes from B_TRUE to P_TRUE while it measures -- 0.6 m and 2 degrees of yaw.
B_TRUE = np.array([0.10, -0.05, 0.02, 0.004, -0.003, 0.010])
P_TRUE = B_TRUE + np.array([0.55, 0.23, 0.03, 0.0, 0.0, np.deg2rad(2.0)])
# 0.1 m and 0.5 degrees.  (From [0.08, -0.05, 0.03] the ORACLE's rigid align of the ideal scan stops after two iterations,
# 0.094 m out -- its line search collapses -- and would be no yardstick for the condition below; from here it runs six.)
GUESS_OFF = np.array([0.06, 0.08, 0.0, 0.0, 0.0, np.deg2rad(0.5)])


def pose_matrices(q):
    T = np.zeros((len(q), 4, 4))
    T[:, :3, :3] = rot_derivs_many(q)[0]
    T[:, :3, 3] = q[:, :3]
    T[:, 3, 3] = 1.0
    return T


@functools.lru_cache(maxsize=None)
def scene(seed=3):
    """Hilly ground and the vertical faces of six buildings on 28 m x 28 m: all six degrees of freedom are held.
    target: 9 000 points; world: 4 500 points of ANOTHER sample of the same surfaces, each with a time factor uniform in
    [0, 1].  raw: what the moving sensor records, x_i = T(p_i*)^-1 w_i in f64 rounded to float32, p_i* the blend of
    B_TRUE and P_TRUE; ideal: the ideally deskewed scan T(P_TRUE)^-1 w_i."""
    from slam_sam_amd import synth
    rng = np.random.default_rng(seed)
    half = 14.0
    boxes = np.stack([rng.uniform(-half + 4, half - 4, 6), rng.uniform(-half + 4, half - 4, 6), rng.uniform(1.5, 3.5, 6),
                      rng.uniform(1.5, 3.5, 6), rng.uniform(3.0, 6.0, 6)], 1)
    tgt = synth._wide_surfaces(rng, 6000, 3000, half, boxes)
    tgt = (tgt + rng.normal(0.0, 0.02, tgt.shape)).astype(np.float32)
    rs = np.random.default_rng(seed + 1)
    world = synth._wide_surfaces(rs, 3000, 1500, half - 2.0, boxes)
    world = world + rs.normal(0.0, 0.02, world.shape)
    alpha = rs.uniform(0.0, 1.0, len(world)).astype(np.float32)
    _, q, _ = ct_point_poses(B_TRUE, P_TRUE, alpha)
    Ti = np.linalg.inv(pose_matrices(q))
    raw = (np.einsum("nab,nb->na", Ti[:, :3, :3], world) + Ti[:, :3, 3]).astype(np.float32)
    truth = synth.pose_matrix(*P_TRUE)
    ideal = synth.transform(np.linalg.inv(truth), world).astype(np.float32)
    return dict(target=tgt, raw=raw, ideal=ideal, alpha=alpha, truth=truth, guess=synth.pose_matrix(*(P_TRUE + GUESS_OFF)))


def oracle_grid(O, cloud, **kw):
    prm = O.default_params(resolution=1.0, num_threads=8, **dict(KW, **kw))
    g = O.Grid(cloud, prm)
    return g, g.export(), dict(min_b=g.min_b, max_b=g.max_b, div_b=g.div_b, leaf_size=1.0)


@pytest.fixture(scope="module")
def side(O, pkg):
    s = scene()
    g, leaves, grid = oracle_grid(O, s["target"])
    assert 300 < len(leaves["mean"]) < 3000
    d1, d2 = gauss_constants(pkg)
    return dict(s, G=g, leaves=leaves, grid=grid, d1=d1, d2=d2)


def restatement_evaluator(pkg, begin, src, alpha, leaves, grid, d1, d2, method="DIRECT7", log=None):
    def ev(pose6, T, need_h):
        r = ct_numpy(begin, pose6, src, alpha, leaves, grid, d1, d2, method, hessian=bool(need_h))
        if log is not None:
            log.append(np.array(pose6))
        return pkg.pack_eval(r["score"], r["gradient"], r["hessian"], r["nvtl_sum"], r["n_with_neighbors"], r["n_pairs"])
    return ev


def newton_over_restatement(pkg, side, log=None):
    ev = restatement_evaluator(pkg, B_TRUE, side["raw"], side["alpha"], side["leaves"], side["grid"], side["d1"], side["d2"], log=log)
    return pkg.newton_align(pkg.default_params(resolution=1.0, **KW), len(side["raw"]), side["guess"], ev)


# ---- the yardstick's own checks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("attitude", [(0.0, 0.0, 0.0), VEHICLE, ATTITUDE], ids=["identity", "vehicle", "far"])
@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT1"])
def test_gradient_and_hessian_are_the_central_differences(pkg, side, attitude, method):
    """step and bound as tests/test_d2d_cpu.py derives them for the same check (the terms are the same Gaussians)"""
    from slam_sam_amd import synth
    d1, d2, leaves, grid = side["d1"], side["d2"], side["leaves"], side["grid"]
    pose = np.array([0.21, -0.13, 0.05, *attitude])
    begin = pose - np.array([0.5, 0.2, -0.04, 0.01, -0.015, 0.03])
    alpha = np.random.default_rng(17).uniform(0.0, 1.0, len(side["ideal"])).astype(np.float32)
    # the source is put where the rotated cloud overlaps the target: rotate it back by the attitude first
    back = np.linalg.inv(synth.pose_matrix(0, 0, 0, *attitude))
    src = synth.transform(back, side["ideal"]).astype(np.float32)
    pairs = d2d_pairs(ct_moved(begin, pose, src, alpha)[2], leaves, grid, method)
    assert len(pairs[0]) > (5000 if method == "DIRECT7" else 1500)
    at = ct_numpy(begin, pose, src, alpha, leaves, grid, d1, d2, method, pairs=pairs)
    assert at["n_pairs"] > 0.9 * len(pairs[0]) and at["score"] > 0
    assert np.abs(at["hessian"] - at["hessian"].T).max() <= 1e-12 * np.abs(at["hessian"]).max()
    g_fd, H_fd = np.zeros(6), np.zeros((6, 6))
    for c in range(6):
        hi, lo = pose.copy(), pose.copy()
        hi[c] += FD_STEP
        lo[c] -= FD_STEP
        rh = ct_numpy(begin, hi, src, alpha, leaves, grid, d1, d2, method, hessian=False, pairs=pairs)
        rl = ct_numpy(begin, lo, src, alpha, leaves, grid, d1, d2, method, hessian=False, pairs=pairs)
        assert rh["n_pairs"] == rl["n_pairs"] == at["n_pairs"]                # the guard cuts the same pairs
        g_fd[c] = (rh["score"] - rl["score"]) / (2 * FD_STEP)
        H_fd[c] = (rh["gradient"] - rl["gradient"]) / (2 * FD_STEP)
    eg = np.linalg.norm(at["gradient"] - g_fd) / np.linalg.norm(at["gradient"])
    eh = np.linalg.norm(at["hessian"] - H_fd) / np.linalg.norm(at["hessian"])
    print("central differences %s %s: gradient %.2e, Hessian %.2e of their norms" % (method, attitude, eg, eh))
    assert eg < FD_TOL and eh < FD_TOL, (eg, eh)
    no_h = ct_numpy(begin, pose, src, alpha, leaves, grid, d1, d2, method, hessian=False, pairs=pairs)
    assert no_h["score"] == at["score"] and np.array_equal(no_h["gradient"], at["gradient"]) and not no_h["hessian"].any()


# the pose of the comparisons with f32-transform arithmetic: identity attitude, a translation of binary fractions
RIGID_POSE = np.array([0.75, 0.25, 0.125, 0.0, 0.0, 0.0])


def rigid_source(side):
    """the ideally deskewed scan turned by the true attitude: RIGID_POSE puts it 0.1 / 0.07 / 0.075 m from the target"""
    from slam_sam_amd import synth
    return synth.transform(synth.pose_matrix(0, 0, 0, *P_TRUE[3:]), side["ideal"]).astype(np.float32)


def face_distance(m, leaf=1.0):
    """the smallest distance of a moved point to a voxel face (NaN rows: points that are not counted)"""
    m = m[np.isfinite(m).all(axis=1)] / leaf
    return float((np.abs(m - np.round(m)) * leaf).min())


def assert_close_all_round(got, want, tol):
    """counters equal; score, nvtl_sum, gradient and Hessian to `tol` of their sizes"""
    assert got["n_pairs"] == want["n_pairs"] and got["n_with_neighbors"] == want["n_with_neighbors"]
    assert got["score"] == pytest.approx(want["score"], rel=tol, abs=1e-12)
    assert got["nvtl_sum"] == pytest.approx(want["nvtl_sum"], rel=tol, abs=1e-12)
    gn, hn = np.linalg.norm(want["gradient"]), np.linalg.norm(want["hessian"])
    assert np.linalg.norm(got["gradient"] - want["gradient"]) <= tol * gn + 1e-12
    assert np.linalg.norm(got["hessian"] - want["hessian"]) <= tol * hn + 1e-12


# At a general attitude the f32-transform side (the oracle, ndt_eval_derivatives) evaluates at a slightly different pose:
# its matrix is built in f32 from f32 products of sin and cos -- two products and a sum per entry, each rounded to half an
# ulp of a number below 1: at most 3 x 2^-24 per entry, 9 x 2^-24 = 5.4e-7 over a row's three entries and the
# translation's rounding, taken as the size dp of a pose perturbation common to all points (metres and radians alike: the
# lever arms of the scene are what the Hessian's rotation block already carries).  A common perturbation dp moves the
# score by at most |g| dp, the gradient by |H| dp, and the Hessian by its own rate of change: each further derivative of
# a pair's term grows it by at most lever arm x d2 |B mu| ~ 35 m x 10 (tests/test_d2d_cpu.py, the central-difference
# note), so |dH| <= 350 |H| dp.  Nothing below 1e-6, the bound where the matrices agree.
F32_POSE_DP, DERIV_GROWTH = 9.0 * 2.0 ** -24, 350.0


def assert_close_to_f32_transform(got, want):
    """counters equal; score / nvtl_sum, gradient and Hessian within what a pose perturbation of F32_POSE_DP explains"""
    gn, hn = np.linalg.norm(want["gradient"]), np.linalg.norm(want["hessian"])
    ts = max(1e-6 * abs(want["score"]), gn * F32_POSE_DP)
    tg = max(1e-6 * gn, hn * F32_POSE_DP)
    th = max(1e-6 * hn, DERIV_GROWTH * hn * F32_POSE_DP)
    es, en = abs(got["score"] - want["score"]), abs(got["nvtl_sum"] - want["nvtl_sum"])
    eg, eh = np.linalg.norm(got["gradient"] - want["gradient"]), np.linalg.norm(got["hessian"] - want["hessian"])
    print("against an f32 transform: score %.2e (bound %.2e), nvtl %.2e, gradient %.2e (bound %.2e), Hessian %.2e (bound %.2e)"
          % (es, ts, en, eg, tg, eh, th))
    assert got["n_pairs"] == want["n_pairs"] and got["n_with_neighbors"] == want["n_with_neighbors"]
    assert es <= ts and en <= ts and eg <= tg and eh <= th


@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT1"])
def test_alpha_one_at_a_vehicle_attitude_is_the_oracles_evaluation(O, side, method):
    """every alpha = 1 at the scan's own attitude (roll 0.004, pitch -0.003, yaw 0.054; 0.1 m and 0.5 degrees from the true
    pose): the f64 per-point rotation against the oracle's independent evaluation, to the bound derived above"""
    pose = P_TRUE + GUESS_OFF
    g, leaves, grid = oracle_grid(O, side["target"], search_method=O.DIRECT7 if method == "DIRECT7" else O.DIRECT1)
    want = g.derivatives(side["ideal"], pose)
    got = ct_numpy(B_TRUE, pose, side["ideal"], np.ones(len(side["ideal"]), np.float32), leaves, grid, side["d1"], side["d2"], method)
    assert got["n_pairs"] > 1000
    assert_close_to_f32_transform(got, want)


@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT1"])
def test_alpha_one_is_the_oracles_evaluation(O, side, method):
    """every alpha = 1: the ordinary point-to-distribution evaluation at p.  The oracle moves the points with the
    reference's f32 matrix (it has no f64 transform mode), so the bound is the 1e-6 that tests/test_gpu_parity.py's
    assert_derivs_match gives gradient and Hessian for reference arithmetic -- here for score and nvtl_sum too: that
    function holds them to 1e-9 because both of its sides move the points in f32, while an f32 matrix puts a point
    6e-8 x 20 m ~ 1e-6 m from where f64 puts it, and a score of ~3e3 with per-point slopes of ~1 moves by ~1e-4.
    The pose is one whose f32 matrix is exact (RIGID_POSE): an f32 rotation matrix is the f64 one turned by ~3e-8 rad, the
    same for every point, which moves the gradient by the Hessian times that -- 5e6 x 3e-8 ~ 0.15 here, 2e-6 of the
    norm -- and says nothing about the rule.  It lies 0.15 m from the scan's true pose, where the gradient is large.
    Precondition on the inputs, as in the D2D tests: no moved point within 1e-6 of a voxel face (at this pose both sides
    round the same sum x + t to f32 once, so they classify alike)."""
    pose, src = RIGID_POSE, rigid_source(side)
    g, leaves, grid = oracle_grid(O, side["target"], search_method=O.DIRECT7 if method == "DIRECT7" else O.DIRECT1)
    want = g.derivatives(src, pose)
    ones = np.ones(len(src), np.float32)
    assert face_distance(ct_moved(B_TRUE, pose, src, ones)[2]) >= 1e-6
    for begin in (B_TRUE, np.array([5.0, -3.0, 1.0, 0.3, 0.2, -1.0])):       # the begin pose plays no part
        got = ct_numpy(begin, pose, src, ones, leaves, grid, side["d1"], side["d2"], method)
        assert got["n_pairs"] > 1000
        print("alpha = 1 against the oracle, %s: gradient %.2e, Hessian %.2e of their norms" % (
            method, np.linalg.norm(got["gradient"] - want["gradient"]) / np.linalg.norm(want["gradient"]),
            np.linalg.norm(got["hessian"] - want["hessian"]) / np.linalg.norm(want["hessian"])))
        assert_close_all_round(got, want, 1e-6)


def test_equal_poses_do_not_see_the_times(side):
    """b == p: every point's pose is p itself whatever its time is, so the points land where the rigid evaluation puts
    them: score, nvtl_sum and the counters are bit-equal for any times.  Gradient and Hessian are NOT independent of the
    times, by the header's own rule: they are the derivatives with respect to the END pose, of which point i follows the
    share a_i (d p_i / d p = a_i I) even where begin and end coincide -- with every alpha = 1 they are the rigid ones, and
    in general the gradient is the a-weighted, the Hessian the a^2-weighted sum of the rigid evaluation's terms."""
    pose = P_TRUE + GUESS_OFF
    n = len(side["raw"])
    rng = np.random.default_rng(2)
    args = (side["leaves"], side["grid"], side["d1"], side["d2"])
    r0 = ct_numpy(pose, pose, side["raw"], np.ones(n, np.float32), *args)
    assert r0["n_pairs"] > 1000
    for alpha in (side["alpha"], rng.permutation(side["alpha"]), np.zeros(n, np.float32), rng.uniform(-1, 2, n).astype(np.float32)):
        r = ct_numpy(pose, pose, side["raw"], alpha, *args)
        assert r["score"] == r0["score"] and r["nvtl_sum"] == r0["nvtl_sum"]
        assert r["n_pairs"] == r0["n_pairs"] and r["n_with_neighbors"] == r0["n_with_neighbors"]
    # one common factor 0.5 (exact in binary): the gradient halves, the Hessian quarters, bit for bit
    half = ct_numpy(pose, pose, side["raw"], np.full(n, 0.5, np.float32), *args)
    assert np.array_equal(half["gradient"], 0.5 * r0["gradient"]) and np.array_equal(half["hessian"], 0.25 * r0["hessian"])
    zero = ct_numpy(pose, pose, side["raw"], np.zeros(n, np.float32), *args)
    assert not zero["gradient"].any() and not zero["hessian"].any()


def test_newton_align_over_the_restatement_converges(pkg, side):
    from slam_sam_amd import synth
    log = []
    r = newton_over_restatement(pkg, side, log)
    dt, dr = synth.pose_error(r["T"], side["truth"])
    print("newton_align over the CT restatement: %d iterations, %d evaluations, %.4f m %.2e rad from the true end pose"
          % (r["iterations"], len(log), dt, dr))
    assert r["converged"] and 1 <= r["iterations"] < 35
    assert dt < 0.05 and dr < 0.005                                           # a twentieth of a leaf, 0.3 degrees


# A rigid align of the raw scan fits one pose to points recorded along 0.6 m and 2 degrees: it lands near the middle of
# the motion, about half of it from the end pose.  A third of that -- 0.1 m, and the same share of the yaw -- is far above
# anything the voxel statistics scatter by, and far below the expected bias.
E_RAW_MIN_M, E_RAW_MIN_RAD = 0.1, np.deg2rad(2.0) / 6.0


def usefulness(pkg, O, side):
    from slam_sam_amd import synth
    rigid = side["G"].align(side["ideal"], side["guess"])
    raw = side["G"].align(side["raw"], side["guess"])
    ct = newton_over_restatement(pkg, side)
    assert rigid["converged"] and raw["converged"] and ct["converged"]
    return tuple(synth.pose_error(r["T"], side["truth"]) for r in (rigid, raw, ct))


def test_continuous_time_removes_the_bias_of_a_rigid_align(pkg, O, side):
    """Measured on the seeded scene (oracle align on the ideally deskewed scan / on the raw scan / Newton over the
    restatement on the raw scan): see DESIGN 7o for the figures this prints."""
    e_rigid, e_raw, e_ct = usefulness(pkg, O, side)
    print("e_rigid %.5f m %.2e rad, e_raw %.5f m %.2e rad, e_ct %.5f m %.2e rad" % (e_rigid + e_raw + e_ct))
    assert e_raw[0] >= E_RAW_MIN_M and e_raw[1] >= E_RAW_MIN_RAD
    assert e_ct[0] <= 4.0 * e_rigid[0] + ALIGN_TOL_M and e_ct[1] <= 4.0 * e_rigid[1] + ALIGN_TOL_RAD


def test_apply_restatement_recovers_the_ideal_scan(side):
    """at the true poses, frame 0 gives the ideally deskewed scan to within f32 rounding of the coordinates (the raw
    scan's own rounding, moved, plus the output's: a few ulp of coordinates below 32 m)"""
    y = ct_apply_numpy(B_TRUE, P_TRUE, side["raw"], side["alpha"], frame=0)
    assert np.abs(y.astype(np.float64) - side["ideal"]).max() < 8 * np.spacing(np.float32(16.0))
    y1 = ct_apply_numpy(B_TRUE, P_TRUE, side["raw"], np.ones_like(side["alpha"]), frame=0)
    assert np.array_equal(y1.view(np.uint32), side["raw"].view(np.uint32))
    y2 = ct_apply_numpy(P_TRUE, P_TRUE, side["raw"], side["alpha"], frame=0)
    assert np.array_equal(y2.view(np.uint32), side["raw"].view(np.uint32))
    # THE FIT: the same two rotations written on other Euler branches deskew to the same scan
    def other(p):
        return np.array([p[0], p[1], p[2], p[3] + np.pi, np.pi - p[4], p[5] + np.pi])
    turn = np.array([0, 0, 0, 0, 0, 2 * np.pi])
    assert np.array_equal(ct_fit_begin(B_TRUE, P_TRUE), B_TRUE)                                  # on the branch: bit for bit
    assert np.abs(ct_fit_begin(other(B_TRUE), P_TRUE) - B_TRUE).max() < 1e-15
    for b, e in ((B_TRUE, other(P_TRUE)), (other(B_TRUE), P_TRUE), (B_TRUE + turn, P_TRUE), (B_TRUE, other(P_TRUE) - turn),
                 (B_TRUE - 3 * turn, other(P_TRUE) + 2 * turn)):
        y = ct_apply_numpy(b, e, side["raw"], side["alpha"], frame=0)
        assert np.abs(y.astype(np.float64) - side["ideal"]).max() < 8 * np.spacing(np.float32(16.0))


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, dp, fp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float)
    want = {
        "ndt_set_source_times": [vp, vp, C.c_size_t],
        "ndt_set_source_times_device": [vp, vp, C.c_size_t],
        "ndt_source_times_info": [vp],
        "ndt_eval_derivatives_ct": [vp, dp, dp, C.c_int, C.c_int, dp],
        "ndt_align_ct": [vp, dp, fp, C.POINTER(pkg.Result)],
        "ndt_transform_source_ct": [vp, dp, dp, C.c_int, vp, C.c_size_t],
        "ndt_transform_source_ct_device": [vp, dp, dp, C.c_int, vp, vp, vp, C.c_size_t],
    }
    for name in NEW:
        assert re.search(r"\bint(?:64_t)?\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    assert L.ndt_source_times_info.restype is C.c_int64
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for decl in ("int ndt_set_source_times(ndt_handle* h, const float* alpha, size_t n);",
                 "int ndt_set_source_times_device(ndt_handle* h, const float* d_alpha, size_t n);",
                 "int64_t ndt_source_times_info(const ndt_handle* h);",
                 "int ndt_eval_derivatives_ct(ndt_handle* h, const double begin_pose6[6], const double* poses6, int K, "
                 "int compute_hessian, double* out);",
                 "int ndt_align_ct(ndt_handle* h, const double begin_pose6[6], const float guess_colmajor[16], ndt_result* out);",
                 "int ndt_transform_source_ct(ndt_handle* h, const double begin_pose6[6], const double end_pose6[6], int frame, "
                 "float* out_xyz, size_t cap_points);",
                 "int ndt_transform_source_ct_device(ndt_handle* h, const double begin_pose6[6], const double end_pose6[6], "
                 "int frame, float* ox, float* oy, float* oz, size_t cap);"):
        assert decl in flat, decl
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    hpp = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    for m in ("setInputSourceTimes", "computeDerivativesCT", "alignContinuousTime", "getDeskewedSource"):
        assert re.search(r"\b%s\s*\(" % m, hpp), m
    for m in ("setSourceTimes", "setSourceTimesDevice", "sourceTimesInfo", "evalDerivativesCT", "alignContinuousTime",
              "transformSourceCT"):
        assert callable(getattr(pkg, m)), m
    mk = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "Makefile")).read()
    assert "$(B)/ndt_ct.o" in mk


def test_argument_errors_come_before_the_handle(pkg):
    L = pkg.lib()
    al = (C.c_float * 2)(0.25, 0.75)
    pose = (C.c_double * 6)()
    nan_pose = (C.c_double * 6)(0, 0, 0, 0, np.nan, 0)
    inf_pose = (C.c_double * 6)(np.inf, 0, 0, 0, 0, 0)
    words = (C.c_double * 32)()
    guess = (C.c_float * 16)()
    xyz = (C.c_float * 6)()
    res = pkg.Result()
    # NULL handle
    assert L.ndt_set_source_times(None, al, 2) == -1
    assert L.ndt_set_source_times_device(None, al, 2) == -1
    assert L.ndt_source_times_info(None) == -1
    assert L.ndt_eval_derivatives_ct(None, pose, pose, 1, 1, words) == -1
    assert L.ndt_align_ct(None, pose, guess, C.byref(res)) == -1
    assert L.ndt_transform_source_ct(None, pose, pose, 0, xyz, 2) == -1
    assert L.ndt_transform_source_ct_device(None, pose, pose, 0, xyz, xyz, xyz, 2) == -1
    # the argument checks come before the handle is looked at: a stand-in block of zero bytes is never read
    h = C.create_string_buffer(1 << 16)
    assert L.ndt_set_source_times(h, None, 2) == -1
    assert L.ndt_set_source_times_device(h, None, 2) == -1
    assert L.ndt_eval_derivatives_ct(h, None, pose, 1, 1, words) == -1
    assert L.ndt_eval_derivatives_ct(h, pose, None, 1, 1, words) == -1
    assert L.ndt_eval_derivatives_ct(h, pose, pose, 1, 1, None) == -1
    assert L.ndt_eval_derivatives_ct(h, pose, pose, 0, 1, words) == -1
    assert L.ndt_eval_derivatives_ct(h, pose, pose, -3, 1, words) == -1
    for bad in (nan_pose, inf_pose):
        assert L.ndt_eval_derivatives_ct(h, bad, pose, 1, 1, words) == -1
        assert L.ndt_eval_derivatives_ct(h, pose, bad, 1, 1, words) == -1
        assert L.ndt_align_ct(h, bad, guess, C.byref(res)) == -1
        assert L.ndt_transform_source_ct(h, bad, pose, 0, xyz, 2) == -1
        assert L.ndt_transform_source_ct(h, pose, bad, 0, xyz, 2) == -1
        assert L.ndt_transform_source_ct_device(h, bad, pose, 0, xyz, xyz, xyz, 2) == -1
        assert L.ndt_transform_source_ct_device(h, pose, bad, 1, xyz, xyz, xyz, 2) == -1
    assert L.ndt_align_ct(h, None, guess, C.byref(res)) == -1
    assert L.ndt_align_ct(h, pose, None, C.byref(res)) == -1
    assert L.ndt_align_ct(h, pose, guess, None) == -1
    assert L.ndt_transform_source_ct(h, None, pose, 0, xyz, 2) == -1
    assert L.ndt_transform_source_ct(h, pose, None, 0, xyz, 2) == -1
    assert L.ndt_transform_source_ct(h, pose, pose, 0, None, 2) == -1
    assert L.ndt_transform_source_ct(h, pose, pose, 2, xyz, 2) == -1                 # frame is 0 or 1
    assert L.ndt_transform_source_ct_device(h, pose, pose, 0, None, xyz, xyz, 2) == -1
    assert L.ndt_transform_source_ct_device(h, pose, pose, 0, xyz, xyz, None, 2) == -1
    assert L.ndt_transform_source_ct_device(h, pose, pose, -1, xyz, xyz, xyz, 2) == -1
    assert bytes(h.raw) == bytes(1 << 16) and not any(words) and not any(xyz)        # nothing was written


def test_python_functions_validate_before_the_library(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)   # no handle: nothing may reach the library
    ndt._h = None
    p6 = np.zeros(6)
    bad = [
        lambda: pkg.setSourceTimes(ndt, np.zeros((3, 2))),
        lambda: pkg.setSourceTimesDevice(ndt, 0, 16),
        lambda: pkg.setSourceTimesDevice(ndt, 4096, -1),
        lambda: pkg.evalDerivativesCT(ndt, np.zeros(5), p6),
        lambda: pkg.evalDerivativesCT(ndt, np.full(6, np.nan), p6),
        lambda: pkg.evalDerivativesCT(ndt, p6, np.zeros(5)),
        lambda: pkg.evalDerivativesCT(ndt, p6, np.full((2, 6), np.inf)),
        lambda: pkg.alignContinuousTime(ndt, np.zeros((4, 4))),
        lambda: pkg.alignContinuousTime(ndt, p6, np.zeros((3, 3))),
        lambda: pkg.alignContinuousTime(ndt, p6, np.full((4, 4), np.nan)),
        lambda: pkg.transformSourceCT(ndt, p6, np.zeros(7)),
        lambda: pkg.transformSourceCT(ndt, np.full(6, np.inf), p6),
        lambda: pkg.transformSourceCT(ndt, p6, p6, frame=2),
        lambda: pkg.transformSourceCTDevice(ndt, p6, p6, 0, 16, 16, 4),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d reached the library" % k)


# ---- the kernels --------------------------------------------------------------------------------------------------------
def test_ct_kernels_do_not_spill(tmp_path):
    """ndt_ct.hip for gfx950: every kernel carries k_ct_, none uses scratch, all stay within the 256 architectural VGPRs;
    no inline assembly and no atomics in the source."""
    path = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_ct.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", ln)
        if m and name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    assert usage and all("k_ct_" in k for k in usage), sorted(usage)
    kernels = {re.search(r"k_ct_[a-z_]+?(?=I|E)", k).group(0) for k in usage}
    assert kernels == {"k_ct_eval", "k_ct_apply"}, kernels
    assert len(usage) == 5                                                            # k_ct_eval: <HESSIAN, D7> four times
    for k, u in usage.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 256, (k, u)
    src = open(path).read()
    assert len(re.findall(r"__global__", src)) == len(kernels)
    assert not re.findall(r"atomic\w*\(", src) and not re.search(r"\basm\b", src)
    # the fixed-order sum and its host driver, the neighbour rule and the block row are the shared ones, not copies
    assert "lane_eval_rows(" in src and "k_eval_rows_sum" not in src.split("namespace ndt")[1]
    assert "neighbor_cells7<" in src and "floorf(" not in src and "eval_block_row<" in src and "__shfl_xor" not in src
