"""GICP's neighbour search, pairing and covariances on the device at the edges of the point index (ndt_fit_device.h,
fit_build_cloud, gicp_knn_point / gicp_pair_point), bit for bit against brute force over all points: coordinates at
+-16 km / +-32 km, cell edges whose reciprocal is inexact in f32, a cell edge that grows, degenerate extents, a finite
neighbour cap that leaves points on both sides without a covariance, queries outside the target's box and queries that
are not finite.  The clouds, and the proof that they are those cases, are tests/test_gicp_edges_cpu.py's.

A point with fewer than k neighbours within reach walks every cell of its index's box (the exact search has no other way
to know); with a grown cell edge that is up to 2^30 cells.  So the growth clouds are searched under an infinite cap only
where every point has k neighbours near by, the cloud with stray points only under a cap of 1 m, and nothing is ever
paired against them; the parameters are set BEFORE the cloud, so that no call derives lists under another rule."""
import numpy as np
import pytest

from test_ct_cpu import ALIGN_TOL_M, ALIGN_TOL_RAD, scene
from test_gicp_cpu import DEFAULTS, GAP_MIN, GAP_SHARE, KS, MIN_NEIGHBOURS, gicp_align_numpy, gicp_numpy, pairs_brute, reg_cov_numpy, sym3
from test_gicp_edges_cpu import (BLOB, CAP_DIAGONAL, CAP_TABLE, CAPS, D_SCENE, DEGENERATE, EDGES, GROWTH_EDGES, GROWTH_KS, LATTICE_SIZES,
                                 OFFSETS, OUTSIDE_CAP, OUTSIDE_K, POSE_GENERAL, brute, cloud_of, index_geometry, lattice_edges,
                                 scene_pairs, scene_setting)
from test_gpu_d2d import assert_matches
from test_gpu_gicp import REG_COV_MEASURED, bits, defaults, engine, same_bits, words_of

pytestmark = pytest.mark.gpu

EPS = DEFAULTS["covariance_epsilon"]
SOURCE_CASES = ([("lattice-%s%s-%d" % (o, "-quarter" if s else "", n), e) for n in LATTICE_SIZES for o in OFFSETS for s in (False, True)
                 for e in lattice_edges(s)] + [("sheet-%s" % o, e) for o in ("km20", "inexact") for e in EDGES + (0.15,)])


@pytest.fixture(scope="module")
def engines(pkg):
    """engines without a target, one per cell edge: the source side needs none (and the dense NDT grid of a target must not
    be asked for the growth clouds' extent)"""
    made = {}

    def get(resolution):
        if resolution not in made:
            made[resolution] = engine(pkg, resolution=resolution)
        return made[resolution]
    return get


def lists_and_moments(pkg, E, name, k, cap):
    """sets the rule, derives, and holds lists, counts, means and raw covariances to brute force bit for bit"""
    want = brute(name, k, cap)
    defaults(pkg, E, k_neighbours=k, max_neighbour_distance=cap)
    idx, found = pkg.gicpNeighbours(E, "source")
    assert idx.shape == want["idx"].shape and np.array_equal(found, want["found"]), (name, k, cap)
    assert np.array_equal(idx, want["idx"]), (name, k, cap, np.nonzero((idx != want["idx"]).any(axis=1))[0][:5])
    cov = pkg.gicpCovariances(E, "source")
    assert same_bits(cov["mean"], want["mean"]) and same_bits(cov["raw_cov6"], want["raw"]), (name, k, cap)
    none = want["found"] < MIN_NEIGHBOURS
    assert np.isnan(cov["cov6"][none]).all() and np.isfinite(cov["cov6"][~none]).all()
    return idx, found, cov


# ---- 1. the source side -----------------------------------------------------------------------------------------------------
WALK_LIMIT = 2_000_000   # cells; the lattice's far point walks its index's whole box once per derivation under an infinite cap


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,edge", SOURCE_CASES, ids=["%s-%s" % c for c in SOURCE_CASES])
def test_neighbours_and_raw_covariances_equal_brute_force(pkg, engines, name, edge, k):
    E = engines(edge)
    defaults(pkg, E)
    E.setInputSource(cloud_of(name))
    caps = (np.inf, 1.0) + ((CAP_DIAGONAL,) if "-quarter" in name else ())
    cheap = index_geometry(cloud_of(name), edge)[3].prod() <= WALK_LIMIT
    for cap in caps:
        first = lists_and_moments(pkg, E, name, k, cap)
        if k == 20 and (cheap or np.isfinite(cap)):
            # to 4 and back to 20: the first answer's bits (the order in which the queue was filled must not show)
            lists_and_moments(pkg, E, name, 4, cap)
            again = lists_and_moments(pkg, E, name, 20, cap)
            assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
            for key in ("mean", "raw_cov6", "cov6"):
                assert same_bits(first[2][key], again[2][key]), (key, cap)
    defaults(pkg, E)


def covariance_conditions(cov, found, plane=False):
    """what holds for the regularised covariance whatever the eigen-solver: symmetric, trace 2 + eps, and the normal n of
    C = I - (1 - eps) n n^T attains the smallest eigenvalue of the engine's own raw covariance"""
    have = found >= MIN_NEIGHBOURS
    Cg, raw = cov["cov"][have], sym3(cov["raw_cov6"][have])
    assert have.any() and np.isfinite(Cg).all()
    assert np.array_equal(bits(Cg), bits(Cg.transpose(0, 2, 1)))
    assert np.abs(np.trace(Cg, axis1=1, axis2=2) - (2.0 + EPS)).max() <= 1e-12
    N = (np.eye(3)[None] - Cg) / (1.0 - EPS)
    lam = np.linalg.eigvalsh(raw)
    quotient = np.einsum("nab,nba->n", raw, N)                                # trace(raw N) = n^T raw n
    assert (quotient <= lam[:, 0] + 1e-12 * np.maximum(lam[:, 2], np.finfo(np.float64).tiny)).all()
    if plane:
        z = np.zeros((3, 3))
        z[2, 2] = 1.0
        assert np.abs(N - z[None]).max() <= 1e-15                             # the normal is +-z


@pytest.mark.parametrize("edge", (1.0, 0.3))
@pytest.mark.parametrize("which", DEGENERATE)
def test_degenerate_extents(pkg, engines, which, edge):
    name = "degenerate-%s" % which
    E = engines(edge)
    defaults(pkg, E)
    E.setInputSource(cloud_of(name))
    for k in KS:
        for cap in (np.inf, 1.0):
            idx, found, cov = lists_and_moments(pkg, E, name, k, cap)
            if which == "five":
                assert found[2] == 0 and (idx[2] == -1).all() and np.isnan(cov["cov6"][2]).all()
            if which in ("four", "five") and np.isinf(cap):
                assert (found[np.isfinite(cloud_of(name)).all(axis=1)] == 4).all()
            if (found >= MIN_NEIGHBOURS).any():
                covariance_conditions(cov, found, plane=which == "plane")
    defaults(pkg, E)


@pytest.mark.parametrize("offset", ("km20", "inexact"))
def test_regularised_covariance_at_km_scale(pkg, engines, offset):
    """against numpy.linalg.eigh of the engine's OWN raw covariance under test_regularised_covariance's rule and bound; the
    raw covariance is taken about the list's mean in f64, so the distance from the origin does not enter it.  Measured on an
    MI355X: largest |C - C_numpy| 1.998e-15 (20 km) and 1.776e-15 (the inexact offset) over 4 099 points, none below the gap:
    within ten times REG_COV_MEASURED as it stands."""
    name = "sheet-%s" % offset
    E = engines(1.0)
    defaults(pkg, E)
    E.setInputSource(cloud_of(name))
    idx, found, got = lists_and_moments(pkg, E, name, 20, np.inf)
    Cn, gap = reg_cov_numpy(got["raw_cov6"], EPS)
    wide = gap >= GAP_MIN
    assert (~wide).mean() <= GAP_SHARE
    dev = float(np.abs(got["cov"][wide] - Cn[wide]).max())
    print("%s: largest |C - C_numpy| %.3e over %d points (%.4f below the gap)" % (name, dev, wide.sum(), (~wide).mean()))
    assert dev <= 10.0 * REG_COV_MEASURED
    covariance_conditions(got, found)


@pytest.mark.parametrize("k", GROWTH_KS)
@pytest.mark.parametrize("edge", GROWTH_EDGES)
def test_grown_cell_edge(pkg, edge, k):
    """two blobs 190 m apart: the cell edge grows (tests/test_gicp_edges_cpu.py pins by how much), every point has its k
    neighbours within 3 cell edges, many of them beyond the 27 cells of pass 1"""
    E = engine(pkg, resolution=edge)
    defaults(pkg, E, k_neighbours=k)                                          # the rule first, then the cloud
    E.setInputSource(cloud_of("growth"))
    idx, found, cov = lists_and_moments(pkg, E, "growth", k, np.inf)
    assert (found == k).all() and ((idx < BLOB) == (np.arange(2 * BLOB) < BLOB)[:, None]).all()
    covariance_conditions(cov, found)


def test_grown_cell_edge_with_strays_under_a_cap(pkg):
    """three stray points between the blobs under a neighbour cap of 1 m: fewer than 4 neighbours, NaN rows, every blob point
    keeps its full list.  (Under an infinite cap each stray would walk the box's 885^3 cells: never run.)"""
    E = engine(pkg, resolution=0.1)
    for k in GROWTH_KS:
        defaults(pkg, E, k_neighbours=k, max_neighbour_distance=1.0)          # the cap first, then the cloud
        E.setInputSource(cloud_of("growth-strays"))
        idx, found, cov = lists_and_moments(pkg, E, "growth-strays", k, 1.0)
        assert (found[:2 * BLOB] == k).all() and (found[2 * BLOB:] < MIN_NEIGHBOURS).all() and (found[2 * BLOB:] >= 1).all()
        without = np.isnan(cov["cov6"]).all(axis=1)
        assert without.sum() == 3 and without[2 * BLOB:].all()                # counted: three rows without a covariance
        assert np.isnan(cov["mean"][2 * BLOB:]).all() and np.isnan(cov["raw_cov6"][2 * BLOB:]).all()


# ---- 2. the target side -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(pkg):
    made = {}

    def get(tname):
        if tname not in made:
            made[tname] = engine(pkg)
            made[tname].setInputTarget(cloud_of(tname))
        return made[tname]
    return get


def paired(pkg, A, setting, cap, D=D_SCENE):
    """the engine on the setting's target with the setting's source under the neighbour cap, paired at the setting's pose"""
    tname, sname, pose = scene_setting(setting)
    defaults(pkg, A, max_neighbour_distance=cap, max_correspondence_distance=D)
    A.setInputSource(cloud_of(sname))
    return pkg.gicpPair(A, pose), cloud_of(tname), cloud_of(sname), pose


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("setting", ("general", "attitude", "shifted"))
def test_pairs_under_a_neighbour_cap_equal_brute_force(pkg, rig, setting, cap):
    """points without a covariance on both sides: `the nearest target point has no covariance: the pair is dropped, not
    replaced by the next nearest` decides for hundreds of pairs at 0.5 m; at POSE_GENERAL, at a far attitude and 3 km out"""
    A = rig(scene_setting(setting)[0])
    want = scene_pairs(setting, cap)
    count, tgt, src, pose = paired(pkg, A, setting, cap)
    for which, key in (("source", "sfound"), ("target", "tfound")):
        _, found = pkg.gicpNeighbours(A, which)
        assert np.array_equal(found, want[key]), which
    idx, d2 = pkg.gicpPairs(A)
    assert count == (want["pair"] >= 0).sum() and np.array_equal(idx, want["pair"]), np.nonzero(idx != want["pair"])[0][:5]
    assert np.array_equal(bits(d2), bits(want["d2"]))
    # dropped for the target point alone: paired when every target point counts as having a covariance
    free, _ = pairs_brute(pose, src, want["sfound"], tgt, np.full(len(tgt), 20, np.int32), D_SCENE)
    dropped = int(((free >= 0) & (idx < 0)).sum())
    print("%s, cap %.1f: %d pairs, %d dropped for the target point alone" % (setting, cap, count, dropped))
    assert dropped == want["dropped_for_target"] and (want["tfound"][free[(free >= 0) & (idx < 0)]] < MIN_NEIGHBOURS).all()
    if cap == 0.5:
        assert dropped >= 100
    if setting == "general":
        t = CAP_TABLE[cap]
        assert count == t["pairs"] and dropped == t["dropped_for_target"]
        assert (want["tfound"] < MIN_NEIGHBOURS).sum() == t["target_without"] and (want["sfound"] < MIN_NEIGHBOURS).sum() == t["source_without"]
        assert np.isnan(pkg.gicpCovariances(A, "target")["cov6"]).all(axis=1).sum() == t["target_without"]
        assert np.isnan(pkg.gicpCovariances(A, "source")["cov6"]).all(axis=1).sum() == t["source_without"]
    defaults(pkg, A)


@pytest.mark.parametrize("shifted", [False, True], ids=["scene", "shifted"])
def test_pairs_of_a_source_outside_the_box(pkg, rig, shifted):
    """queries 40 m outside the target's box on every side and 1e6 m out: the clamps k = -1 and k = dims and the dG terms of
    the bound on every axis.  The source's own lists are taken with k = 4 under a cap of 200 m (see outside_source)."""
    tname, sname = ("scene-target-shifted", "outside-shifted") if shifted else ("scene-target", "outside")
    A = rig(tname)
    defaults(pkg, A, k_neighbours=OUTSIDE_K, max_neighbour_distance=OUTSIDE_CAP)   # the rule first, then the cloud
    A.setInputSource(cloud_of(sname))
    S, T = brute(sname, OUTSIDE_K, OUTSIDE_CAP), brute(tname, OUTSIDE_K, OUTSIDE_CAP)
    idx, found = pkg.gicpNeighbours(A, "source")
    assert np.array_equal(idx, S["idx"]) and np.array_equal(found, S["found"]) and (found == OUTSIDE_K).all()
    src, tgt = cloud_of(sname), cloud_of(tname)
    # a rotation about the origin would carry the shifted source 90 m off: the second pose turns only where the scene is near it
    poses = (np.zeros(6), np.array([0.3, -0.2, 0.1, 0.0, 0.0, 0.0]) if shifted else np.array([0.3, -0.2, 0.1, 0.01, -0.02, 0.03]))
    # a D whose f32 square IS the d2 of the point 40 m out on +x at the identity pose: the inclusive rule decides
    at_inf = pairs_brute(poses[0], src, S["found"], tgt, T["found"], np.inf)[1]
    D_on = float(np.sqrt(np.float64(at_inf[0])))
    while np.float32(D_on * D_on) < at_inf[0]:
        D_on = float(np.nextafter(D_on, np.inf))
    assert np.float32(D_on * D_on) == at_inf[0] and 20.0 < D_on < 40.0
    for D in (np.inf, D_SCENE, D_on):
        defaults(pkg, A, k_neighbours=OUTSIDE_K, max_neighbour_distance=OUTSIDE_CAP, max_correspondence_distance=D)
        for pose in poses:
            count = pkg.gicpPair(A, pose)
            got, d2 = pkg.gicpPairs(A)
            want, want_d2 = pairs_brute(pose, src, S["found"], tgt, T["found"], D)
            assert count == (want >= 0).sum() and np.array_equal(got, want), (D, np.nonzero(got != want)[0][:5])
            assert np.array_equal(bits(d2), bits(want_d2))
            if np.isinf(D):
                assert count == 32 and d2[14:22].min() > 1e11
            elif D == D_SCENE:
                assert (got[:22] == -1).all() and (got[22:] >= 0).all()
            elif pose is poses[0]:
                assert got[0] >= 0 and d2[0] == np.float32(D_on * D_on)       # exactly on the cap: kept
    defaults(pkg, A, k_neighbours=OUTSIDE_K, max_neighbour_distance=OUTSIDE_CAP,
             max_correspondence_distance=float(np.sqrt(np.float64(np.nextafter(at_inf[0], np.float32(0))))) * (1.0 - 1e-9))
    pkg.gicpPair(A, poses[0])
    assert pkg.gicpPairs(A)[0][0] == -1                                       # one f32 step below: dropped
    defaults(pkg, A)


def test_queries_that_are_not_finite(pkg, rig):
    """a translation beyond f32: every moved point is infinite, nothing is paired, and the call succeeds"""
    A = rig("scene-target")
    defaults(pkg, A)
    A.setInputSource(cloud_of("scene-source"))
    for D in (D_SCENE, np.inf):
        defaults(pkg, A, max_correspondence_distance=D)
        assert pkg.gicpPair(A, [3.5e38, 0, 0, 0, 0, 0]) == 0
        idx, d2 = pkg.gicpPairs(A)
        assert len(idx) == 4500 and (idx == -1).all() and np.isposinf(d2).all()
    defaults(pkg, A)
    assert pkg.gicpPair(A, POSE_GENERAL) > 4000                               # and the engine goes on


@pytest.mark.parametrize("setting,cap", [("general", 0.5), ("attitude", np.inf)], ids=["cap-0.5", "attitude"])
def test_evaluation_equals_the_restatement(pkg, rig, setting, cap):
    A = rig("scene-target")
    count, tgt, src, base = paired(pkg, A, setting, cap)
    pair, _ = pkg.gicpPairs(A)
    assert count == (pair >= 0).sum() > 2000
    sc, tc = pkg.gicpCovariances(A, "source")["cov"], pkg.gicpCovariances(A, "target")["cov"]
    if np.isfinite(cap):
        assert np.isnan(sc).any() and np.isnan(tc).any() and count == CAP_TABLE[cap]["pairs"]
    poses = base[None, :] + np.random.default_rng(5).uniform(-0.02, 0.02, (8, 6))
    poses[0] = base
    got = pkg.evalDerivativesGICP(A, poses)
    for k in (0, 3):
        want = gicp_numpy(poses[k], src, sc, tgt, tc, pair)
        assert_matches(got[k], want)
        assert got[k]["nvtl_sum"] == got[k]["score"] and want["n_pairs"] == count and got[k]["score"] < 0
    # gradient-only: the Hessian call's score and gradient, zero Hessian words
    w_h, w_g = words_of(pkg, A, poses), words_of(pkg, A, poses, hessian=False)
    assert np.array_equal(w_h[:, :7], w_g[:, :7]) and not w_g[:, 7:28].any() and np.array_equal(w_h[:, 28:], w_g[:, 28:])
    assert_matches(pkg.evalDerivativesGICP(A, poses[3], compute_hessian=False)[0], gicp_numpy(poses[3], src, sc, tgt, tc, pair, hessian=False))
    # the same bits every time, and a pose in a batch the bits it gets alone
    assert np.array_equal(words_of(pkg, A, poses), w_h)
    for k in range(8):
        assert np.array_equal(words_of(pkg, A, poses[k])[0], w_h[k]), k
    defaults(pkg, A)


def test_a_pair_whose_q_is_not_finite_contributes_nothing(pkg, rig):
    """pairs frozen at POSE_GENERAL; at a translation of 1e200 m every q overflows: the pose's words are zero and no pair is
    counted, and its neighbours in the batch get the bits they get alone.  At 1e100 m q is finite and every pair counts."""
    A = rig("scene-target")
    count, tgt, src, _ = paired(pkg, A, "general", np.inf)
    assert count > 4000
    batch = np.stack([POSE_GENERAL, [1e200, 0, 0, 0, 0, 0], POSE_GENERAL])
    for hessian in (True, False):
        raw = pkg.evalDerivativesGICP(A, batch, compute_hessian=hessian, raw=True)
        assert (raw[1] == 0.0).all()
        alone = words_of(pkg, A, POSE_GENERAL, hessian=hessian)[0]
        w = raw.view(np.uint64)
        assert np.array_equal(w[0], alone) and np.array_equal(w[2], alone) and alone.any()
    got = pkg.evalDerivativesGICP(A, batch)
    assert got[1]["n_pairs"] == 0 and got[1]["n_with_neighbors"] == 0 and got[1]["score"] == 0.0
    assert got[0]["n_pairs"] == count == got[2]["n_pairs"]
    some = pkg.evalDerivativesGICP(A, [1e100, 0, 0, 0, 0, 0])[0]
    assert some["n_pairs"] == count and np.isfinite(some["score"]) and some["score"] < -1e199
    defaults(pkg, A)


def test_align_under_a_neighbour_cap(pkg, rig):
    """cap 0.8 m: 23 target points and 167 source points without a covariance; the align follows the two-level loop over the
    restatement by test_align_follows_the_loop_over_the_restatement's rules"""
    from slam_sam_amd import synth
    s = scene()
    A = rig("scene-target")
    defaults(pkg, A, max_neighbour_distance=0.8)
    A.setInputSource(s["ideal"])
    T, r = pkg.alignGICP(A, s["guess"])
    info = r["gicp"]
    sc, tc = pkg.gicpCovariances(A, "source"), pkg.gicpCovariances(A, "target")
    _, sfound = pkg.gicpNeighbours(A, "source")
    _, tfound = pkg.gicpNeighbours(A, "target")
    ref = gicp_align_numpy(pkg, s["ideal"], sc["cov"], sfound, s["target"], tc["cov"], tfound, s["guess"])
    dt, dr = synth.pose_error(T, ref["T"])
    print("alignGICP under cap 0.8: %d outer / %d inner iterations, %d pairs (restatement %d outer, inner %s, %d pairs); %.2e m %.2e rad from it"
          % (info["outer_iterations"], info["inner_iterations"], info["n_pairs"], ref["outer"], ref["inner"], ref["n_pairs"], dt, dr))
    assert r["converged"] and ref["converged"] and r["iterations"] == info["outer_iterations"]
    assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD
    assert abs(info["outer_iterations"] - ref["outer"]) <= 1
    slack = 1 + (max(ref["inner"]) if info["outer_iterations"] != ref["outer"] else 0)
    assert abs(info["inner_iterations"] - sum(ref["inner"])) <= slack
    t = CAP_TABLE[0.8]
    assert info["n_source_without_covariance"] == t["source_without"] == 167 and info["n_target_without_covariance"] == t["target_without"] == 23
    assert info["n_pairs"] > 4000
    e_guess, e_gicp = synth.pose_error(s["guess"], s["truth"]), synth.pose_error(T, s["truth"])
    assert e_gicp[0] < e_guess[0] and e_gicp[1] < e_guess[1]
    defaults(pkg, A)
