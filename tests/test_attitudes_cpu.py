"""Attitudes away from the identity, host side: the scenes and the attitude table tests/test_gpu_attitudes.py runs on, the
yardstick checked first (the oracle's gradient against central differences of its own score, and enough pairs at every
attitude), then the host routines that had only run within 0.15 rad of the identity -- the Newton driver from large-attitude
guesses, ndt_angle_tables over the whole table and on both sides of its 1e-7 snap, and the SE(3) logarithm of ndt_se3.h
(through ndt_svn_rbf_kernel) at relative rotations from 1e-8 rad to pi - 1e-7.  None of this needs a GPU.

A scene is one of the project's two smallest clouds seen from another attitude: for a wanted pose
P' = pose_matrix(t, roll, pitch, yaw) the source is src' = inv(P') guess src, computed in f64 and rounded once to f32, so
P' does to src' what the configuration's guess does to its source and the aligned pose is gt inv(guess) P'.  The target
stays where it is."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from test_abi_cpu import angle_tables, check_angle_tables, oracle_evaluator

PI = float(np.pi)
H = PI / 2
KW = dict(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=35)   # every engine and oracle of both modules
ORACLE_THREADS = 16

# name -> (roll, pitch, yaw) in rad
GENERAL = {"general-a": (0.7, -0.5, 2.0), "general-b": (-1.1, 0.9, -2.6), "general-c": (2.8, -1.3, 0.4)}
YAW_WRAP = {"yaw+pi/2": (0.0, 0.0, H), "yaw-pi/2": (0.0, 0.0, -H), "yaw+pi-": (0.0, 0.0, PI - 1e-3),
            "yaw-pi+": (0.0, 0.0, -(PI - 1e-3)), "yaw-f32-pi": (0.02, -0.01, float(np.float32(np.pi)))}
GIMBAL = {"pitch+h-1e-3": (0.3, H - 1e-3, -0.8), "pitch-h+1e-3": (0.3, -(H - 1e-3), -0.8),
          "pitch+h-1e-6": (0.3, H - 1e-6, -0.8), "pitch-h+1e-6": (0.3, -(H - 1e-6), -0.8), "pitch+h": (0.3, H, -0.8)}
FOLD = {"roll+0.3": (0.3, 0.4, -0.6), "roll-0.3": (-0.3, 0.4, -0.6), "roll+pi-": (PI - 1e-3, 0.4, -0.6),
        "roll-pi+": (-(PI - 1e-3), 0.4, -0.6)}
SNAP_VALUES = {"0": 0.0, "+0.9e-7": 0.9e-7, "-0.9e-7": -0.9e-7, "+1.1e-7": 1.1e-7, "-1.1e-7": -1.1e-7}
SNAP_BASE = (0.4, -0.6, 0.5)       # the two angles that are not at the snap keep their entry of this triple


def _snap(axis, v):
    a = list(SNAP_BASE)
    a[axis] = v
    return tuple(a)


SNAP = {"snap-%s%s" % (("roll", "pitch", "yaw")[ax], k): _snap(ax, v) for ax in range(3) for k, v in SNAP_VALUES.items()}
ATTITUDES = {**GENERAL, **YAW_WRAP, **GIMBAL, **FOLD, **SNAP}
# the attitudes an align starts from (the two nearest the gimbal corner and the corner itself are evaluation-only: there
# the Euler angles of a f32 matrix are not determined)
ALIGN = list(GENERAL) + list(YAW_WRAP) + list(FOLD) + ["pitch+h-1e-3", "pitch-h+1e-3"]
# translation of P' (m): one per group, so that no two groups share a source cloud by accident
TRANSLATION = {**{k: (0.6, -0.4, 0.3) for k in GENERAL}, **{k: (-0.5, 0.7, 0.2) for k in YAW_WRAP},
               **{k: (0.3, 0.2, -0.4) for k in GIMBAL}, **{k: (-0.2, -0.6, 0.5) for k in FOLD},
               **{k: (0.45, 0.35, -0.25) for k in SNAP}}
SCENES = ("c1", "g1")


@functools.lru_cache(maxsize=None)
def base_scene(name):
    """C1 (10 k / 10 k) or golden g1 (3 k / 3 k): source, target, gt, guess"""
    import __graft_entry__ as ge
    S = ge.load_package().synth
    if name == "c1":
        cfg = S.config_c1()
        return dict(source=cfg["source"], target=cfg["target"], gt=cfg["gt"], guess=cfg["guess"])
    z = np.load(os.path.join(ge.ROOT, "tests", "golden", "g1_two_plane_3k.npz"))
    _, _, gt, guess = S.two_planes(seed=2024, max_points=3000)       # (test_oracle.py pins the file to this generator)
    np.testing.assert_allclose(guess, z["guess"], atol=1e-15)
    return dict(source=z["source"], target=z["target"], gt=gt, guess=guess)


@functools.lru_cache(maxsize=None)
def scene_at(name, angles, t):
    """The scene `name` seen from the pose (t, angles): dict(source, target, P, pose6, aligned)."""
    import __graft_entry__ as ge
    S = ge.load_package().synth
    b = base_scene(name)
    P = S.pose_matrix(*t, *angles)
    M = np.linalg.inv(P) @ b["guess"]
    src = (b["source"].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    src.setflags(write=False)
    return dict(source=src, target=b["target"], P=P, pose6=np.array([*t, *angles]),
                aligned=b["gt"] @ np.linalg.inv(b["guess"]) @ P)


def scene(name, att):
    return scene_at(name, ATTITUDES[att], TRANSLATION[att])


@functools.lru_cache(maxsize=None)
def oracle_grid(name):
    import __graft_entry__ as ge
    O = ge.load_oracle()
    return O.Grid(base_scene(name)["target"], O.default_params(num_threads=ORACLE_THREADS, pair_mode=2, **KW))


# ------------------------------------------------------------------------------------------------ 6. the yardstick first
@pytest.mark.parametrize("name", SCENES)
def test_every_attitude_keeps_the_pairs_of_the_guess(O, name):
    """A condition of the comparisons, not a measurement: the oracle finds at P' on src' at least half the pairs it finds
    at the unrotated guess, so no case compares zeros.  (src' is the guess's cloud moved back by inv(P'); what differs is
    one f32 rounding of the coordinates and the f32 matrix of the pose.)"""
    grid = oracle_grid(name)
    b = base_scene(name)
    n0 = grid.derivatives(b["source"], O.matrix_to_pose(b["guess"]), T=b["guess"], compute_hessian=False)["n_pairs"]
    assert n0 > 1000
    for att in ATTITUDES:
        s = scene(name, att)
        d = grid.derivatives(s["source"], s["pose6"], compute_hessian=False)
        assert 2 * d["n_pairs"] >= n0, (att, d["n_pairs"], n0)
        # ... and the engine's other way in, the matrix itself with the Euler angles taken from it
        d = grid.derivatives(s["source"], O.matrix_to_pose(s["P"]), T=s["P"], compute_hessian=False)
        assert 2 * d["n_pairs"] >= n0, (att, "by matrix", d["n_pairs"], n0)


@pytest.mark.parametrize("att", list(GENERAL) + list(GIMBAL))
def test_oracle_gradient_is_the_finite_difference_of_its_score(O, S, att):
    """tests/test_oracle.py::test_gradient_hessian_vs_finite_differences away from the identity: on the frozen pair set
    of the pose, the oracle's gradient against central differences of a NumPy restatement of its own score (1e-5 of the
    norm) and its Hessian against Richardson-extrapolated second differences (2e-4, without the entry that carries the
    reference's h_ang row-6 sign) -- at the general attitudes and up to the gimbal corner."""
    s = scene("g1", att)
    src = s["source"][::2].copy()
    grid = O.Grid(s["target"], O.default_params(resolution=1.0))
    L = grid.export()
    p0 = s["pose6"]
    d1, d2, _ = O.gauss_constants(1.0, 0.55)
    T0 = O.pose_to_matrix(p0)
    xt = (src.astype(np.float64) @ T0[:3, :3].T + T0[:3, 3]).astype(np.float32)
    pi, li = [], []
    for i, x in enumerate(xt):
        for r in grid.neighbors(x):
            pi.append(i)
            li.append(r)
    pi, li = np.array(pi), np.array(li)

    def score(p):  # smooth: the pair set is frozen
        X = src[pi].astype(np.float64) @ S.rot_xyz(*p[3:]).T + p[:3]
        xr = X - L["mean"][li]
        q = np.einsum("ni,nij,nj->n", xr, L["icov"][li], xr)
        return np.sum(-d1 * np.exp(-d2 * q / 2))

    d = grid.derivatives(src, p0)
    assert d["n_pairs"] == len(pi) > 500
    # (the oracle transforms with the f32 matrix of the pose, the restatement with the f64 one: 1e-7 in the points)
    assert d["score"] == pytest.approx(score(p0), rel=1e-5)
    E, h = np.eye(6), 1e-5
    g_fd = np.array([(score(p0 + h * e) - score(p0 - h * e)) / (2 * h) for e in E])
    eg = np.linalg.norm(g_fd - d["gradient"]) / np.linalg.norm(g_fd)

    def second_differences(h):
        return np.array([[(score(p0 + h * E[i] + h * E[j]) - score(p0 + h * E[i] - h * E[j])
                           - score(p0 - h * E[i] + h * E[j]) + score(p0 - h * E[i] - h * E[j])) / (4 * h * h)
                          for j in range(6)] for i in range(6)])

    # With a 10 m lever arm over voxel sigmas of centimetres each derivative in an angle costs a factor of some hundred,
    # and with three mid-sized angles the h^2 term of the second difference at test_oracle.py's h = 1e-4 is of the size
    # of the bound itself.  It is taken out by one Richardson step, same bound -- after showing that it is an h^2 term:
    # halving h twice, the differences change fourfold each time.
    H1, H2, H4 = second_differences(1e-4), second_differences(5e-5), second_differences(2.5e-5)
    ratio = np.linalg.norm(H1 - H2) / np.linalg.norm(H2 - H4)
    print("%s: h^2 term of the second differences at h = 1e-4: %.1e of the norm, ratio on halving %.2f"
          % (att, 4.0 / 3.0 * np.linalg.norm(H1 - H2) / np.linalg.norm(H2), ratio))
    assert 3.5 < ratio < 4.5, ratio
    H_fd = (4.0 * H2 - H1) / 3.0
    diff = np.abs(H_fd - d["hessian"]) / np.linalg.norm(H_fd)
    diff[4, 4] = 0.0  # carries the reference's h_ang_d1 sign (test_oracle.py::test_angle_tables_vs_numeric)
    print("%s: gradient %.2e of its norm from central differences, Hessian %.2e" % (att, eg, diff.max()))
    assert eg < 1e-5
    assert diff.max() < 2e-4


# ------------------------------------------------------------------------------------------------ 7. ndt_newton_align
@pytest.mark.parametrize("line_search", [1, 0])
@pytest.mark.parametrize("att", ALIGN)
def test_newton_driver_follows_the_oracle_from_large_attitudes(pkg, O, att, line_search):
    """tests/test_abi_cpu.py::test_newton_driver_matches_oracle_trajectory from guesses all over SO(3): the same
    evaluations in, the product's host loop (matrix_to_pose with its fold at a positive first Euler angle, pose_to_matrix
    in every trial, More-Thuente) takes the oracle's steps."""
    s = scene("g1", att)
    src, guess = s["source"], s["P"]
    kw = dict(KW, use_line_search=line_search)
    oprm = O.default_params(symmetrize_hessian=1, **kw)
    grid = O.Grid(s["target"], oprm)
    ref = grid.align(src, guess)
    log = []
    got = pkg.newton_align(pkg.default_params(**kw), len(src), guess, oracle_evaluator(pkg, O, grid, src, oprm, log))
    assert got["converged"] == ref["converged"]
    assert got["iterations"] == ref["iterations"] > 0
    assert got["n_evaluations"] == ref["n_evaluations"] == len(log)
    np.testing.assert_allclose(got["pose"], ref["pose"], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(got["T"].astype(np.float32), ref["T"].astype(np.float32))
    np.testing.assert_allclose(got["hessian"], ref["hessian"], rtol=1e-12)
    assert got["score"] == pytest.approx(ref["score"], rel=1e-12)
    assert got["nvtl"] == pytest.approx(ref["nvtl"], rel=1e-12)
    for pose, T, _ in log[1:]:
        np.testing.assert_array_equal(T.astype(np.float32), O.pose_to_matrix(pose).astype(np.float32))
    np.testing.assert_array_equal(log[0][1].astype(np.float32), np.asarray(guess, np.float32))
    np.testing.assert_allclose(log[0][0], O.matrix_to_pose(guess), atol=1e-12)
    # the Euler angles the loop starts from are angles of the guess's rotation (either of the two equivalent triples)
    np.testing.assert_allclose(O.pose_to_matrix(log[0][0])[:3, :3], guess[:3, :3], atol=2e-6)


@pytest.mark.parametrize("att", list(GIMBAL))
def test_matrix_to_pose_at_the_gimbal_corner(pkg, O, att):
    """c2 -> 0: the angles of the f32 matrix are badly determined there, but what the host loop takes from them must be
    the oracle's to the bit, finite, and give the rotation back as well as f32 allows (c2 = 1e-3: roll and yaw to
    6e-8 / 1e-3; nearer the corner only their combination is determined, and the matrix is what is compared)."""
    s = scene("g1", att)
    seen = []

    def ev(pose, T, need_h):
        seen.append((pose.copy(), T.copy()))
        raise RuntimeError("one evaluation is all this test wants")

    with pytest.raises(pkg.NdtError):
        pkg.newton_align(pkg.default_params(**KW), len(s["source"]), s["P"], ev)
    pose, T = seen[0]
    assert np.isfinite(pose).all()
    np.testing.assert_allclose(pose, O.matrix_to_pose(s["P"]), atol=1e-12)
    np.testing.assert_array_equal(T.astype(np.float32), s["P"].astype(np.float32))
    # (the bound of tests/test_oracle.py::test_pose_matrix_roundtrip)
    err = np.abs(O.pose_to_matrix(pose)[:3, :3] - s["P"][:3, :3]).max()
    print("%s: pose %s, rotation back within %.1e" % (att, pose[3:], err))
    assert err < 2e-6


# ------------------------------------------------------------------------------------------------ 8. ndt_angle_tables
@pytest.mark.parametrize("att", list(ATTITUDES))
def test_angle_tables_at_every_attitude(pkg, O, att):
    L = pkg.lib()
    check_angle_tables(L, ATTITUDES[att])
    # the oracle's tables are the library's, entry by entry
    p = [0.0, 0.0, 0.0, *ATTITUDES[att]]
    j, h = angle_tables(L, p)
    oj, oh = O.angle_tables(p)
    assert np.array_equal(j, oj) and np.array_equal(h, oh)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_angle_tables_on_both_sides_of_the_snap(pkg, axis):
    """|angle| < 1e-7 is taken as 0 (svn_ndt_impl.hpp:264): at +-0.9e-7 every entry has the bits of the entry at 0, at
    +-1.1e-7 some entry differs (the sine of the angle is there: 1.1e-7 against 0)."""
    L = pkg.lib()

    def bits(v):
        j, h = angle_tables(L, [0.1, 0.2, 0.3, *_snap(axis, v)])
        return np.concatenate([j.ravel(), h.ravel()]).view(np.uint32)

    zero = bits(0.0)
    for v in (0.9e-7, -0.9e-7, 0.99999e-7):
        assert np.array_equal(bits(v), zero), v
    for v in (1.1e-7, -1.1e-7, 1e-7):                    # (the comparison is strict: 1e-7 itself is not snapped)
        assert not np.array_equal(bits(v), zero), v
    assert not np.array_equal(bits(1.1e-7), bits(-1.1e-7))


# ------------------------------------------------------------------------------------------------ 9. ndt_svn_rbf_kernel
def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def se3_exp(xi):
    """Exp of [omega, v] in f64, every coefficient in a form that does not cancel at small or large angles."""
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = np.linalg.norm(w)
    K = _skew(w)
    if th < 1e-4:
        A, B, Cc = 1 - th ** 2 / 6, 0.5 - th ** 2 / 24, 1 / 6 - th ** 2 / 120
    else:
        A, B = np.sin(th) / th, 2 * np.sin(th / 2) ** 2 / th ** 2
        Cc = (1 - A) / th ** 2
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * K + B * (K @ K)
    T[:3, 3] = (np.eye(3) + B * K + Cc * (K @ K)) @ v
    return T


RBF_ANGLES = {"1e-8": 1e-8, "1e-3": 1e-3, "pi-1e-3": PI - 1e-3, "pi-1e-7": PI - 1e-7}
RBF_AXES = {"z": (0.0, 0.0, 1.0), "x": (1.0, 0.0, 0.0), "general": (0.48, -0.6, 0.64), "general-": (-0.36, 0.8, -0.48)}
# the oracle's logarithm restates gtsam's: within 1e-5 rad^2 of pi (trace + 1 < 1e-10) it returns the angle pi itself and
# an axis with a non-negative z (or y, or x) component -- off by pi - theta in the angle and, for half of the axes, by the
# sign.  The identity exp(log(E)) = E decides: the library meets it to 2e-13 at every angle, the oracle to 1e-7 there.
ORACLE_LOG_COARSE = ("pi-1e-7",)


def rbf_log(pkg, Lp, Kp, h=64.0):
    """Log(l^-1 k) as ndt_svn_rbf_kernel computes it, recovered from the kernel's value and gradient (grad = k (-2 / h) Log)"""
    L = pkg.lib()
    dp = C.POINTER(C.c_double)
    L.ndt_svn_rbf_kernel.argtypes = [dp, dp, C.c_double, dp, dp]
    a = np.ascontiguousarray(np.asarray(Lp, np.float64).T).ravel()
    b = np.ascontiguousarray(np.asarray(Kp, np.float64).T).ravel()
    k, g = C.c_double(), np.zeros(6)
    assert L.ndt_svn_rbf_kernel(a.ctypes.data_as(dp), b.ctypes.data_as(dp), h, C.byref(k), g.ctypes.data_as(dp)) == 0
    d = g * (-h / 2.0) / k.value
    assert k.value == pytest.approx(np.exp(-(d @ d) / h), rel=1e-12)
    return d


@pytest.mark.parametrize("axis", list(RBF_AXES))
@pytest.mark.parametrize("angle", list(RBF_ANGLES))
def test_rbf_kernel_logarithm_from_tiny_angles_to_pi(pkg, O, S, angle, axis):
    """se3::between / logmap (so3_log's series, generic and theta ~ pi branches; logmap's D series switch) behind their
    only callable face.  E = l^-1 k has the rotation angle `angle` about `axis`; Log(E) must give E back through an
    independent f64 exponential to 1e-12, and agrees with the oracle's logarithm as far as the oracle's own arithmetic
    carries (1e-12; 3e-9 at pi - 1e-3).  At pi - 1e-7 the two disagree, and the identity says the library is right."""
    n = np.array(RBF_AXES[axis])
    assert abs(np.linalg.norm(n) - 1) < 1e-12
    xi = np.concatenate([RBF_ANGLES[angle] * n, [0.3, -0.2, 0.1]])
    E = se3_exp(xi)
    assert np.abs(E[:3, :3] @ E[:3, :3].T - np.eye(3)).max() < 1e-15
    for Lp in (np.eye(4), S.pose_matrix(0.6, -0.4, 0.3, *GENERAL["general-a"]), S.pose_matrix(-3.0, 2.0, 1.0, *GENERAL["general-c"])):
        Kp = Lp @ E
        Eb = np.linalg.inv(Lp) @ Kp                      # what between() sees, rounding of the two products included
        d = rbf_log(pkg, Lp, Kp)
        resid = np.abs(se3_exp(d) - Eb).max()
        od = O.se3_logmap(Eb)
        oresid = np.abs(se3_exp(od) - Eb).max()
        print("%s about %s: exp(log(E)) - E: library %.1e, oracle %.1e; library - oracle %.1e; library - xi %.1e"
              % (angle, axis, resid, oresid, np.abs(d - od).max(), np.abs(d - xi).max()))
        assert resid < 1e-12
        assert np.abs(d - xi).max() < 1e-9                # the principal logarithm: the tangent E was made from
        assert np.linalg.norm(d[:3]) <= PI
        delta = PI - RBF_ANGLES[angle]
        if angle in ORACLE_LOG_COARSE:
            # the oracle's share, not the library's: pi for pi - delta, and the axis by its sign convention
            assert oresid < 4 * delta
            assert min(np.abs(d[:3] - od[:3]).max(), np.abs(d[:3] + od[:3]).max()) < 4 * delta
        else:
            # the oracle takes theta = acos((trace - 1) / 2) and divides by 2 sin(theta): rounding of the trace (1e-16)
            # comes back as 1e-16 / sin(theta) in theta and as 1e-16 pi / sin(theta)^2 in the logarithm -- 3e-10 at
            # pi - 1e-3, nothing at the small angles (there it switches to a series)
            tol = 1e-12 + (1e-15 * PI / np.sin(RBF_ANGLES[angle]) ** 2 if delta < 1.0 else 0.0)
            assert oresid < tol and np.abs(d - od).max() < tol, (oresid, np.abs(d - od).max(), tol)
        # antisymmetry, which ndt_svn_align relies on to evaluate each pair once
        np.testing.assert_allclose(rbf_log(pkg, Kp, Lp), -d, rtol=0, atol=1e-12)
