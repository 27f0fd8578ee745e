"""GPU parity tests: the HIP path, called through the C-ABI, against the CPU oracle on the
same seeded inputs, against the committed golden vectors, and -- at BASELINE.json's full
sizes -- through size-independent properties.

Tolerances (written where used):
  * voxel membership, point counts, neighbour counts: BIT-EXACT (integer work);
  * voxel mean: 1e-12 relative; covariance / inverse: 1e-9 of the matrix' largest entry
    (f64 sums in a different association; at km-scale coordinates the reference's own
    single-pass cancellation bounds it at ~1e-4, see the shifted case);
  * score 1e-9 relative; gradient / Hessian 1e-6 of their norms (the oracle rounds the
    per-pair products to f32 as the reference does, the kernel keeps f64);
  * final transform: <= 1 mm and <= 0.1 mrad from the oracle, and the
    reference test's own 0.05 m / 0.035 rad from ground truth.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALIGN_TOL_M, ALIGN_TOL_RAD = 1e-3, 1e-4


def make_ndt(pkg, **kw):
    n, info = pkg.backend_info()
    assert n > 0, "GPU test on a box without a HIP device: " + info
    base = dict(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=50)
    base.update(kw)
    return pkg.NormalDistributionsTransform(device_id=0, **base)


def assert_leaves_match(L, OL, cov_rtol=1e-9):
    assert np.array_equal(L["cell"], OL["cell"])
    assert np.array_equal(L["count"], OL["count"])
    np.testing.assert_allclose(L["mean"], OL["mean"], rtol=1e-12, atol=0)
    for k in ("cov", "icov"):
        scale = np.abs(OL[k]).max(axis=(1, 2), keepdims=True)
        assert (np.abs(L[k] - OL[k]) / scale).max() < (cov_rtol if k == "cov" else 100 * cov_rtol), k
    scale = np.abs(OL["evals"]).max(axis=1, keepdims=True)
    assert (np.abs(L["evals"] - OL["evals"]) / scale).max() < 100 * cov_rtol


def assert_derivs_match(e, d, tol=1e-6):
    assert e["n_pairs"] == d["n_pairs"]
    assert e["n_with_neighbors"] == d["n_with_neighbors"]
    assert e["score"] == pytest.approx(d["score"], rel=1e-9, abs=1e-9)
    assert e["nvtl_sum"] == pytest.approx(d["nvtl_sum"], rel=1e-9, abs=1e-9)
    gn, hn = np.linalg.norm(d["gradient"]), np.linalg.norm(d["hessian"])
    assert np.linalg.norm(e["gradient"] - d["gradient"]) <= tol * gn + 1e-12
    assert np.linalg.norm(e["hessian"] - d["hessian"]) <= tol * hn + 1e-12


# ---------------------------------------------------------------------------------------
# golden vectors through the HIP path
# ---------------------------------------------------------------------------------------
def test_golden_g1_through_hip(pkg, golden_dir):
    z = np.load(os.path.join(golden_dir, "g1_two_plane_3k.npz"))
    ndt = make_ndt(pkg)
    ndt.setInputTarget(z["target"])
    gi = ndt.getGridInfo()
    assert np.array_equal(gi["min_b"], z["min_b"]) and np.array_equal(gi["div_b"], z["div_b"])
    L = ndt.getLeaves()
    assert_leaves_match(L, dict(cell=z["leaf_cell"], count=z["leaf_count"], mean=z["leaf_mean"],
                                cov=z["leaf_cov"], icov=z["leaf_icov"], evals=z["leaf_evals"]))
    ndt.setInputSource(z["source"])
    for i, e in enumerate(ndt.evalDerivatives(z["poses"])):
        assert_derivs_match(e, dict(score=z["score"][i], gradient=z["gradient"][i], hessian=z["hessian"][i],
                                    n_pairs=z["n_pairs"][i], n_with_neighbors=z["n_with"][i],
                                    nvtl_sum=z["nvtl_sum"][i]))
    T = ndt.align(z["guess"])
    r = ndt.getResult()
    assert r["converged"] == bool(z["align_converged"])
    dt, dr = pkg.synth.pose_error(T, z["align_T"])
    assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD
    # variants
    ndt.setParams(hessian_mode=pkg.HESSIAN_GAUSS_NEWTON, add_ridge=1)
    e = ndt.evalDerivatives(z["poses"][0])[0]
    np.testing.assert_allclose(e["hessian"], z["gn_hessian"], rtol=0, atol=1e-6 * np.linalg.norm(z["gn_hessian"]))
    ndt.setParams(hessian_mode=pkg.HESSIAN_FULL, add_ridge=0, search_method=pkg.DIRECT1)
    e = ndt.evalDerivatives(z["poses"][0])[0]
    assert e["n_pairs"] == int(z["d1_n_pairs"])
    np.testing.assert_allclose(e["gradient"], z["d1_gradient"], rtol=0, atol=1e-6 * np.linalg.norm(z["d1_gradient"]))


# ---------------------------------------------------------------------------------------
# the reference's own test, through the product
# ---------------------------------------------------------------------------------------
def test_reference_convergence_test_through_hip(pkg, O, S):
    """ConvergenceComparison.PclOmp (ref: test_svn_ndt.cpp:138-199) with the HIP engine."""
    src, tgt, gt, guess = O.two_plane_fixture()
    ndt = make_ndt(pkg, resolution=1.0, max_iterations=50, trans_epsilon=1e-4, step_size=0.1)
    ndt.setNeighborhoodSearchMethod(pkg.DIRECT7)
    ndt.setNumThreads(20)
    ndt.setInputTarget(tgt)
    ndt.setInputSource(src)
    T = ndt.computeTransformation(guess)
    assert ndt.hasConverged()
    assert ndt.getFinalNumIteration() < 50
    trans_err, rot_err = S.se3_log_error(T, gt)
    assert trans_err < 0.05 and rot_err < 0.035
    ref = O.Grid(tgt, O.default_params(resolution=1.0, max_iterations=50, trans_epsilon=1e-4, step_size=0.1)).align(src, guess)
    dt, dr = S.pose_error(T, ref["T"])
    assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD


# ---------------------------------------------------------------------------------------
# configuration-level parity
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2(S):
    return S.config_c2()


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_config_parity(pkg, O, S, c2, name):
    cfg = S.config_c1() if name == "c1" else c2
    res = float(cfg["resolution"])
    prm = O.default_params(resolution=res, step_size=0.1, trans_epsilon=1e-4, max_iterations=35, num_threads=8)
    grid = O.Grid(cfg["target"], prm)
    ndt = make_ndt(pkg, resolution=res, max_iterations=35)
    ndt.setInputTarget(cfg["target"])
    assert_leaves_match(ndt.getLeaves(), grid.export())
    ndt.setInputSource(cfg["source"])
    p0 = O.matrix_to_pose(cfg["guess"])
    poses = np.stack([p0, p0 + [0.05, -0.03, 0.02, 0.01, -0.005, 0.008], O.matrix_to_pose(cfg["gt"])])
    prm64 = O.default_params(resolution=res, step_size=0.1, trans_epsilon=1e-4, max_iterations=35, num_threads=8,
                             pair_mode=2)   # test seam: the reference's formulas with f64 products
    for p, e in zip(poses, ndt.evalDerivatives(poses)):
        assert_derivs_match(e, grid.derivatives(cfg["source"], p))                       # reference arithmetic: 1e-6
        assert_derivs_match(e, grid.derivatives(cfg["source"], p, params=prm64), 1e-9)   # same formulas in f64: 1e-9
    # single-pose launch path (kernel-argument pose) must agree with the batched one bit for bit
    e1 = ndt.evalDerivatives(poses[1])[0]
    eb = ndt.evalDerivatives(poses)[1]
    assert e1["score"] == eb["score"] and np.array_equal(e1["hessian"], eb["hessian"])
    T = ndt.align(cfg["guess"])
    r = ndt.getResult()
    ref = grid.align(cfg["source"], cfg["guess"])
    assert r["converged"] and ref["converged"]
    dt, dr = S.pose_error(T, ref["T"])
    assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD, (dt, dr)
    gt_t, gt_r = S.pose_error(T, cfg["gt"])
    assert gt_t < 0.05 and gt_r < 0.035
    # covariance the drivers derive from the result: -(H + 1e-6 I)^-1 (ref: run/pipeline.cpp:594-596)
    cov = -np.linalg.inv(r["hessian"] + 1e-6 * np.eye(6))
    cov_ref = -np.linalg.inv(ref["hessian"] + 1e-6 * np.eye(6))
    assert np.linalg.norm(cov - cov_ref) < 1e-2 * np.linalg.norm(cov_ref)
    # output cloud of align(): source transformed by the result
    out = ndt.transformSource(T)
    expect = S.transform(T, cfg["source"])
    assert np.abs(out - expect).max() < 1e-4


def test_km_scale_coordinates(pkg, O, S):
    """+3 km offset (NED-scale): exercises f32 index arithmetic and f64 statistics."""
    cfg = S.config_c1()
    off = np.array([3000.0, -2000.0, 100.0], np.float32)
    tgt = (cfg["target"] + off).astype(np.float32)
    shift = np.eye(4)
    shift[:3, 3] = off
    guess, gt = shift @ cfg["guess"], shift @ cfg["gt"]
    prm = O.default_params(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=50)
    grid = O.Grid(tgt, prm)
    ndt = make_ndt(pkg)
    ndt.setInputTarget(tgt)
    # the reference's single-pass covariance loses ~|mu|^2 eps / sigma^2 here: compare at 1e-4
    assert_leaves_match(ndt.getLeaves(), grid.export(), cov_rtol=1e-6)
    ndt.setInputSource(cfg["source"])
    p = O.matrix_to_pose(guess)
    assert_derivs_match(ndt.evalDerivatives(p)[0], grid.derivatives(cfg["source"], p), tol=1e-5)
    T = ndt.align(guess)
    # At 3 km one f32 ulp is 0.24 mm: every transformed point is quantised at that level (the
    # reference transforms in f32 too, ref: svn_ndt_impl.hpp:761), so the score is a staircase in
    # the pose and the fixture's weak direction (both planes contain the x axis) turns any last-bit
    # difference into a different More-Thuente decision.  The oracle shows this on itself, without
    # a GPU: its own two arithmetics -- the reference's f32 per-pair products (pair_mode 0) and the
    # same formulas in f64 (pair_mode 2) -- end 12.1 mm apart here and 0.07 mm apart at the origin
    # (tests/test_oracle.py::test_km_scale_gap_is_the_references_f32_products).  The kernel
    # carries f64, so it is held to the f64 trajectory at the 1 mm / 0.1 mrad of SURVEY 8c, and
    # to the reference-arithmetic one at that measured 12 mm (+ margin).
    prm64 = O.default_params(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=50, pair_mode=2)
    ref64 = grid.align(cfg["source"], guess, params=prm64)
    dt, dr = S.pose_error(T, ref64["T"])
    assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD, (dt, dr)
    assert ndt.getResult()["iterations"] == ref64["iterations"]
    ref = grid.align(cfg["source"], guess)
    gap_t, gap_r = S.pose_error(ref64["T"], ref["T"])   # the oracle against itself
    dt, dr = S.pose_error(T, ref["T"])
    assert dt < gap_t + ALIGN_TOL_M and dr < gap_r + ALIGN_TOL_RAD, (dt, dr, gap_t, gap_r)
    assert ndt.getResult()["score"] == pytest.approx(ref["score"], rel=2e-3)
    assert S.pose_error(T, gt)[0] < 0.05 and S.pose_error(ref["T"], gt)[0] < 0.05


@pytest.mark.parametrize("name", ["c2", "c3_50k"])
def test_km_scale_on_non_degenerate_geometry(pkg, O, S, name):
    """the +3 km case above is the two-plane fixture, whose x direction is free.  The same
    shift (+3 km, -2 km, +100 m: the drivers' NED map frame, ref: run/pipeline.cpp:554-556) on geometry where no
    direction is free -- the C2 street canyon, and a 50 k-point subsample of the C3 scan against the full 1 M-point
    map: leaves vs the oracle, derivatives at three poses, align against the oracle in BOTH pair modes.  Here the
    oracle's two arithmetics agree to 1e-12 m (tests/test_oracle.py::test_km_scale_gap_vanishes_on_non_degenerate
    _geometry), so the kernel is held to the reference-arithmetic trajectory at the full 1 mm / 0.1 mrad too: the
    12 mm of the two-plane case is a property of that fixture, not of km-scale coordinates."""
    # tolerances of the voxel statistics and of the derivatives at 3 km (explained below): the cancellation of the
    # single-pass covariance grows with |mu|^2 / sigma^2, i.e. 4x from 1.0 m voxels (C2) to 0.5 m voxels (C3)
    if name == "c2":
        cfg, res = S.config_c2(), 1.0
        src = cfg["source"]
        cov_rtol, score_rel, gh_tol = 1e-6, 1e-6, 1e-5
    else:
        cfg, res = S.config_c3(), 0.5
        src = cfg["source"][np.random.default_rng(5).choice(len(cfg["source"]), 50000, replace=False)]
        cov_rtol, score_rel, gh_tol = 1e-5, 1e-5, 1e-4
    off = np.array([3000.0, -2000.0, 100.0])
    tgt = (cfg["target"].astype(np.float64) + off).astype(np.float32)
    shift = np.eye(4)
    shift[:3, 3] = off
    guess, gt = shift @ cfg["guess"], shift @ cfg["gt"]
    kw = dict(resolution=res, step_size=0.1, trans_epsilon=1e-4, max_iterations=35)
    prm = O.default_params(num_threads=8, **kw)
    grid = O.Grid(tgt, prm)
    ndt = make_ndt(pkg, **kw)
    ndt.setInputTarget(tgt)
    # the reference's single-pass covariance loses ~|mu|^2 eps / sigma^2 at 3 km (membership, counts: bit-exact; means 1e-12)
    assert_leaves_match(ndt.getLeaves(), grid.export(), cov_rtol=cov_rtol)
    ndt.setInputSource(src)
    mid = shift @ S.pose_matrix(*(0.5 * (O.matrix_to_pose(cfg["guess"]) + O.matrix_to_pose(cfg["gt"]))))
    prm64 = O.default_params(num_threads=8, pair_mode=2, **kw)
    # Derivatives: at 3 km the voxel statistics themselves carry ~1e-6 of relative noise -- the reference's single-pass
    # covariance sum(x x^T) / n - mu mu^T in f64 of f32 coordinates of 3e3 m cancels seven digits, so the ORDER of the
    # moment sums shows (the oracle adds in input order, the kernel in a fixed tree; a C2 voxel holds up to 924 points,
    # the two-plane fixture's <= 32 sum exactly).  Pair membership and counts stay bit-exact; score / g / H are held
    # at 1e-6 / 1e-5 (1.0 m voxels) and 1e-5 / 1e-4 (0.5 m voxels) here against 1e-9 / 1e-6 at the origin.
    for T0 in (guess, gt, mid):
        p = O.matrix_to_pose(T0)
        e = ndt.evalDerivatives(p)[0]
        for d in (grid.derivatives(src, p), grid.derivatives(src, p, params=prm64)):   # f32 products / the same in f64
            assert e["n_pairs"] == d["n_pairs"] and e["n_with_neighbors"] == d["n_with_neighbors"]
            assert e["score"] == pytest.approx(d["score"], rel=score_rel)
            assert np.linalg.norm(e["gradient"] - d["gradient"]) <= gh_tol * np.linalg.norm(d["gradient"]) + 1e-9
            assert np.linalg.norm(e["hessian"] - d["hessian"]) <= gh_tol * np.linalg.norm(d["hessian"]) + 1e-9
    T = ndt.align(guess)
    it = ndt.getResult()["iterations"]
    for params in (prm64, prm):
        ref = grid.align(src, guess, params=params)
        dt, dr = S.pose_error(T, ref["T"])
        assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD, (name, dt, dr)
        # (the 1e-6 noise of the statistics may move one stopping decision: 16 against 17 iterations on C3)
        assert abs(it - ref["iterations"]) <= 1
    assert S.pose_error(T, gt)[0] < 0.05


def test_parameter_variants(pkg, O, S):
    cfg = S.config_c1()
    p = O.matrix_to_pose(cfg["guess"])
    for kw, okw in (
        (dict(resolution=2.0), dict(resolution=2.0)),
        (dict(resolution=0.5, min_points_per_voxel=3), dict(resolution=0.5, min_points_per_voxel=3)),
        (dict(cov_mode=1), dict(cov_mode=1)),
        (dict(outlier_ratio=0.3), dict(outlier_ratio=0.3)),
        (dict(search_method=3), dict(search_method=1)),
        (dict(hessian_mode=1, add_ridge=1), dict(hessian_mode=1, add_ridge=1)),
        (dict(eig_inflation_ratio=0.1), dict(eig_inflation_ratio=0.1)),
    ):
        grid = O.Grid(cfg["target"], O.default_params(**okw))
        ndt = make_ndt(pkg, **kw)
        ndt.setInputTarget(cfg["target"])
        ndt.setInputSource(cfg["source"])
        assert_leaves_match(ndt.getLeaves(), grid.export())
        assert_derivs_match(ndt.evalDerivatives(p)[0], grid.derivatives(cfg["source"], p))
        ndt.close()


def test_kdtree_search_mode(pkg, O, S, c2):
    """setNeighborhoodSearchMethod(KDTREE) (ref: run/pipeline.cpp:475-476): radius search over the
    voxel centroids, on the GPU as a 27-cell scan; neighbour sets must match the oracle exactly."""
    for cfg, res in ((S.config_c1(), 1.0), (c2, 1.0)):
        grid = O.Grid(cfg["target"], O.default_params(resolution=res, search_method=O.KDTREE, step_size=0.1,
                                                      trans_epsilon=1e-4, max_iterations=35, num_threads=8))
        ndt = make_ndt(pkg, resolution=res, max_iterations=35)
        ndt.setNeighborhoodSearchMethod(pkg.KDTREE)
        ndt.setInputTarget(cfg["target"])
        ndt.setInputSource(cfg["source"])
        p0 = O.matrix_to_pose(cfg["guess"])
        poses = np.stack([p0, O.matrix_to_pose(cfg["gt"]), O.matrix_to_pose(S.pose_matrix(400, 0, 0, 0, 0, 0))])
        for p, e in zip(poses, ndt.evalDerivatives(poses)):
            assert_derivs_match(e, grid.derivatives(cfg["source"], p))
        T = ndt.align(cfg["guess"])
        ref = grid.align(cfg["source"], cfg["guess"])
        dt, dr = S.pose_error(T, ref["T"])
        assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD
        ndt.close()


def test_regularization_and_fixed_step(pkg, O, S):
    cfg = S.config_c1()
    reg_pose = cfg["gt"] @ S.pose_matrix(0.05, 0.0, 0.0, 0, 0, 0)
    kw = dict(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=40)
    oprm = O.default_params(use_regularization=1, regularization_scale_factor=0.01,
                            regularization_pose=reg_pose, use_line_search=0, **kw)
    grid = O.Grid(cfg["target"], oprm)
    ndt = make_ndt(pkg, use_line_search=0, **{k: v for k, v in kw.items() if k != "resolution"})
    ndt.setRegularizationScaleFactor(0.01)
    ndt.setRegularizationPose(reg_pose)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    p = O.matrix_to_pose(cfg["guess"])
    assert_derivs_match(ndt.evalDerivatives(p)[0], grid.derivatives(cfg["source"], p))
    T = ndt.align(cfg["guess"])
    ref = grid.align(cfg["source"], cfg["guess"])
    dt, dr = S.pose_error(T, ref["T"])
    assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD
    assert abs(ndt.getFinalNumIteration() - ref["iterations"]) <= 2  # stop test |step| < eps sits on rounding


# ---------------------------------------------------------------------------------------
# the voxel build's hand-written radix sort: bit-exact against a stable argsort
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bits,kind", [
    (1, 1, "uniform"), (63, 5, "uniform"), (64, 8, "uniform"), (4096, 8, "uniform"), (4097, 9, "uniform"),
    (8191, 16, "uniform"), (100000, 17, "uniform"), (1000003, 23, "uniform"), (1000003, 23, "runs"),
    (300000, 24, "skewed"), (250000, 31, "uniform"), (250000, 32, "uniform"), (70000, 12, "constant"),
    (500000, 23, "reversed"),
])
def test_radix_sort_is_stable_and_exact(pkg, n, bits, kind):
    rng = np.random.default_rng(n * 131 + bits)
    hi = (1 << bits) - 1
    if kind == "uniform":
        keys = rng.integers(0, hi, n, dtype=np.uint64, endpoint=True)
    elif kind == "runs":      # scan-order-like: long runs of equal keys, few distinct values (voxel ids)
        keys = np.repeat(rng.integers(0, hi, n // 40 + 1, dtype=np.uint64), 40)[:n]
    elif kind == "skewed":    # a handful of heavy cells + a sentinel tail
        keys = np.where(rng.random(n) < 0.7, rng.integers(0, 16, n), rng.integers(0, hi, n, endpoint=True)).astype(np.uint64)
        keys[rng.random(n) < 0.05] = hi
    elif kind == "constant":
        keys = np.full(n, hi // 3, np.uint64)
    else:                     # strictly descending
        keys = (hi - np.arange(n, dtype=np.uint64)) & hi
    keys = keys.astype(np.uint32)
    ndt = make_ndt(pkg)
    ko, vo = ndt.debugSortPairs(keys, bits)
    perm = np.argsort(keys, kind="stable")
    assert np.array_equal(vo, perm.astype(np.uint32))
    assert np.array_equal(ko, keys[perm])


# ---------------------------------------------------------------------------------------
# edge cases (empty, ragged, non-finite, no overlap, input layouts)
# ---------------------------------------------------------------------------------------
def test_edge_cases(pkg, O, S):
    cfg = S.config_c1()
    ndt = make_ndt(pkg)
    # align before any cloud: loud status, prior returned
    with pytest.raises(pkg.NdtError) as ei:
        ndt.align(cfg["guess"])
    assert ei.value.code == -4
    # empty target / target without a valid voxel
    with pytest.raises(pkg.NdtError):
        ndt.setInputTarget(np.zeros((0, 3), np.float32))
    ndt.setInputTarget(np.random.default_rng(0).uniform(-50, 50, (200, 3)).astype(np.float32))
    assert ndt.getGridInfo()["n_leaves"] == 0
    ndt.setInputSource(cfg["source"])
    with pytest.raises(pkg.NdtError) as ei:
        ndt.align(cfg["guess"])
    assert ei.value.code == -4
    # non-finite points in both clouds are skipped exactly as the oracle skips them
    tgt = cfg["target"].copy()
    tgt[::17] = np.nan
    tgt[5::29, 1] = np.inf
    src = cfg["source"].copy()
    src[3::11, 2] = np.nan
    grid = O.Grid(tgt, O.default_params(resolution=1.0))
    ndt.setInputTarget(tgt)
    assert_leaves_match(ndt.getLeaves(), grid.export())
    ndt.setInputSource(src)
    p = O.matrix_to_pose(cfg["guess"])
    assert_derivs_match(ndt.evalDerivatives(p)[0], grid.derivatives(src, p))
    # no overlap: zero score, zero iterations, converged like the oracle
    far = S.pose_matrix(500.0, 0, 0, 0, 0, 0)
    e = ndt.evalDerivatives(O.matrix_to_pose(far))[0]
    assert e["n_pairs"] == 0 and e["score"] == 0.0 and not e["gradient"].any()
    ndt.align(far)
    assert ndt.getFinalNumIteration() == 0
    # ragged sizes: 1 point, 63, 64, 65, 257 points
    for n in (1, 63, 64, 65, 257):
        ndt.setInputSource(cfg["source"][:n])
        assert_derivs_match(ndt.evalDerivatives(p)[0], grid.derivatives(cfg["source"][:n], p))
    # grid overflow guard (ref: voxel_grid_covariance_impl.hpp:108-125)
    huge = np.array([[0, 0, 0], [4e6, 4e6, 4e6]], np.float32)
    tiny = make_ndt(pkg, resolution=0.01)
    with pytest.raises(pkg.NdtError) as ei:
        tiny.setInputTarget(huge)
    assert ei.value.code == -6


def test_rejected_first_leaf_does_not_poison_sums(pkg, O, S):
    """An absent neighbour is evaluated against record 0 and masked with f = 0; record 0 must then
    be finite even when leaf 0 was rejected (here: eight identical points in the lowest cell, zero
    covariance), or 0 * NaN reaches the sums.  Found by the randomised sweep."""
    cfg = S.config_c1()
    lo = cfg["target"].min(axis=0) - 3.0
    tgt = np.concatenate([np.repeat(lo[None, :], 8, axis=0), cfg["target"]]).astype(np.float32)
    kw = dict(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=30)
    grid = O.Grid(tgt, O.default_params(**kw))
    OL = grid.export()
    assert 0 not in OL["cell"]           # the lowest cell (slot 0 of the build) is rejected and erased (ref :307, :341)
    ndt = make_ndt(pkg, **kw)
    ndt.setInputTarget(tgt)
    assert_leaves_match(ndt.getLeaves(), OL)
    ndt.setInputSource(cfg["source"])
    p = O.matrix_to_pose(cfg["guess"])
    for method, omethod in ((pkg.DIRECT7, O.DIRECT7), (pkg.DIRECT1, O.DIRECT1), (pkg.KDTREE, O.KDTREE)):
        ndt.setParams(search_method=method)
        e = ndt.evalDerivatives(p)[0]
        assert np.isfinite(e["gradient"]).all() and np.isfinite(e["hessian"]).all()
        assert_derivs_match(e, grid.derivatives(cfg["source"], p, params=O.default_params(search_method=omethod, **kw)))


def test_two_engines_in_two_threads(pkg, S):
    """One engine per thread, as the reference's drivers run them (an NDT odometry thread beside
    an SVN / map thread): two handles driven concurrently give exactly the single-threaded results
    (process-wide launch tags, per-handle streams and buffers)."""
    import threading
    cfgs = [S.config_c1(), S.config_c2()]
    kw = [dict(resolution=float(c["resolution"]), step_size=0.1, trans_epsilon=1e-4, max_iterations=35) for c in cfgs]

    def run(i, out, reps):
        ndt = pkg.NormalDistributionsTransform(device_id=0, **kw[i])
        res = []
        for _ in range(reps):
            ndt.setInputTarget(cfgs[i]["target"])
            ndt.setInputSource(cfgs[i]["source"])
            ndt.align(cfgs[i]["guess"])
            r = ndt.getResult()
            res.append((r["T"].copy(), r["score"], r["iterations"]))
        out[i] = res

    ref = [None, None]
    for i in range(2):
        run(i, ref, 1)
    got = [None, None]
    th = [threading.Thread(target=run, args=(i, got, 12)) for i in range(2)]
    for t in th: t.start()
    for t in th: t.join()
    for i in range(2):
        assert got[i] is not None and len(got[i]) == 12
        for T, score, it in got[i]:
            assert np.array_equal(T, ref[i][0][0]) and score == ref[i][0][1] and it == ref[i][0][2]


def test_input_layouts_agree(pkg, S):
    """packed xyz, PCL-style 32-byte AoS (PointXYZI) and SoA inputs give identical results."""
    cfg = S.config_c1()
    ndt = make_ndt(pkg)

    def run():
        return ndt.getLeaves(), ndt.evalDerivatives([0.4, 0.0, 0.3, 0.0, 0.05, 0.2])[0]

    ndt.setInputTarget(cfg["target"]); ndt.setInputSource(cfg["source"])
    L0, e0 = run()
    aos_t = np.zeros((len(cfg["target"]), 8), np.float32); aos_t[:, :3] = cfg["target"]; aos_t[:, 4] = 7.0
    aos_s = np.zeros((len(cfg["source"]), 8), np.float32); aos_s[:, :3] = cfg["source"]
    ndt.setInputTarget(aos_t); ndt.setInputSource(aos_s)
    L1, e1 = run()
    ndt.setInputTargetSoA(*cfg["target"].T); ndt.setInputSourceSoA(*cfg["source"].T)
    L2, e2 = run()
    for L, e in ((L1, e1), (L2, e2)):
        assert np.array_equal(L["cell"], L0["cell"]) and np.array_equal(L["cov"], L0["cov"])
        assert e["score"] == e0["score"] and np.array_equal(e["hessian"], e0["hessian"])


def test_set_resolution_rebuilds_target(pkg, O, S):
    """setResolution on a loaded target re-voxelises it (ref: svn_ndt_impl.hpp:162-176)."""
    cfg = S.config_c1()
    ndt = make_ndt(pkg, resolution=1.0)
    ndt.setInputTarget(cfg["target"])
    n1 = ndt.getGridInfo()["n_leaves"]
    ndt.setResolution(2.0)
    grid = O.Grid(cfg["target"], O.default_params(resolution=2.0))
    assert ndt.getGridInfo()["n_leaves"] == grid.n_leaves != n1
    assert_leaves_match(ndt.getLeaves(), grid.export())


# ---------------------------------------------------------------------------------------
# full-size workload (C3: 200k -> 1M, 0.5 m): size-independent properties + oracle spot checks
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3(S):
    return S.config_c3()


@pytest.fixture(scope="module")
def c3_ndt(pkg, c3):
    ndt = make_ndt(pkg, resolution=0.5, max_iterations=35)
    ndt.setInputTarget(c3["target"])
    ndt.setInputSource(c3["source"])
    return ndt


def test_full_size_leaves_and_derivatives_vs_oracle(pkg, O, S, c3, c3_ndt):
    prm = O.default_params(resolution=0.5, step_size=0.1, trans_epsilon=1e-4, max_iterations=35, num_threads=16)
    grid = O.Grid(c3["target"], prm)
    assert_leaves_match(c3_ndt.getLeaves(), grid.export())
    p = O.matrix_to_pose(c3["guess"])
    assert_derivs_match(c3_ndt.evalDerivatives(p)[0], grid.derivatives(c3["source"], p))
    T = c3_ndt.align(c3["guess"])
    ref = grid.align(c3["source"], c3["guess"])
    dt, dr = S.pose_error(T, ref["T"])
    assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD, (dt, dr)
    assert S.pose_error(T, c3["gt"])[0] < 0.05


def test_full_size_determinism_and_idempotence(pkg, O, c3, c3_ndt):
    p = O.matrix_to_pose(c3["guess"])
    a = c3_ndt.evalDerivatives(p)[0]
    b = c3_ndt.evalDerivatives(p)[0]
    assert a["score"] == b["score"] and np.array_equal(a["gradient"], b["gradient"]) and np.array_equal(a["hessian"], b["hessian"])
    T1 = c3_ndt.align(c3["guess"]); r1 = c3_ndt.getResult()
    T2 = c3_ndt.align(c3["guess"]); r2 = c3_ndt.getResult()
    assert np.array_equal(T1, T2) and r1["iterations"] == r2["iterations"] and r1["n_evaluations"] == r2["n_evaluations"]
    L1 = c3_ndt.getLeaves()
    c3_ndt.setInputTarget(c3["target"])  # rebuild: bit-identical statistics
    L2 = c3_ndt.getLeaves()
    for k in ("cell", "count", "mean", "cov", "icov"):
        assert np.array_equal(L1[k], L2[k]), k


def test_full_size_linearity_over_shards(pkg, O, c3, c3_ndt):
    """The evaluation is a sum over source points: shards add up, order does not matter."""
    p = O.matrix_to_pose(c3["guess"])
    full = c3_ndt.evalDerivatives(p)[0]
    src = c3["source"]
    for world in (2, 3, 8):
        acc = None
        for r in range(world):
            b, c = pkg.shard_range(len(src), r, world)
            c3_ndt.setInputSource(src[b:b + c])
            e = c3_ndt.evalDerivatives(p)[0]
            acc = e if acc is None else {k: acc[k] + e[k] for k in e}
        assert acc["n_pairs"] == full["n_pairs"] and acc["n_with_neighbors"] == full["n_with_neighbors"]
        assert acc["score"] == pytest.approx(full["score"], rel=1e-12)
        assert np.linalg.norm(acc["hessian"] - full["hessian"]) < 1e-11 * np.linalg.norm(full["hessian"])
    perm = np.random.default_rng(0).permutation(len(src))
    c3_ndt.setInputSource(src[perm])
    e = c3_ndt.evalDerivatives(p)[0]
    assert e["n_pairs"] == full["n_pairs"]
    assert np.linalg.norm(e["hessian"] - full["hessian"]) < 1e-11 * np.linalg.norm(full["hessian"])
    c3_ndt.setInputSource(src)


def test_large_source_two_level_final_sum(pkg, O, c3, c3_ndt):
    """> 1M source points: more than 2048 partial rows, so the in-kernel final sum goes through
    its group level.  Must equal the sum of the single-level evaluations of its chunks."""
    src = c3["source"]
    rng = np.random.default_rng(5)
    chunks = [(src + rng.normal(0, 0.01, src.shape)).astype(np.float32) for _ in range(6)]
    p = O.matrix_to_pose(c3["gt"])
    acc = None
    for ch in chunks:
        c3_ndt.setInputSource(ch)
        e = c3_ndt.evalDerivatives(p)[0]
        acc = e if acc is None else {k: acc[k] + e[k] for k in e}
    big = np.concatenate(chunks)
    assert len(big) == 1200000
    c3_ndt.setInputSource(big)
    e = c3_ndt.evalDerivatives(p)[0]          # batched kernel
    assert e["n_pairs"] == acc["n_pairs"] and e["n_with_neighbors"] == acc["n_with_neighbors"]
    assert e["score"] == pytest.approx(acc["score"], rel=1e-12)
    assert np.linalg.norm(e["hessian"] - acc["hessian"]) < 1e-11 * np.linalg.norm(acc["hessian"])
    # single-pose kernel at the same grid size: align's last evaluation re-done by the batched one
    c3_ndt.setParams(max_iterations=0)
    c3_ndt.align(c3["gt"])
    r = c3_ndt.getResult()
    eg = c3_ndt.evalDerivatives(r["pose"], transforms=[r["T"]])[0]
    assert r["n_pairs"] == eg["n_pairs"] and r["score"] == eg["score"]
    assert np.array_equal(r["hessian"], eg["hessian"])
    c3_ndt.setParams(max_iterations=35)
    c3_ndt.setInputSource(src)


def test_full_size_leaf_invariants(c3_ndt):
    """Checksum-of-checksums style invariants of the voxel table."""
    L = c3_ndt.getLeaves()
    gi = c3_ndt.getGridInfo()
    assert len(L["cell"]) == gi["n_leaves"] > 1000
    assert (np.diff(L["cell"]) > 0).all()                       # sorted, unique
    assert (L["count"] >= 6).all() and L["count"].sum() <= gi["n_target_points"]
    assert np.abs(L["mean"] - L["center"]).max() <= 0.25 + 1e-4  # mean inside its voxel (leaf/2)
    eye = np.einsum("nij,njk->nik", L["cov"], L["icov"])
    assert np.abs(eye - np.eye(3)).max() < 1e-6
    ev = L["evals"]
    assert (ev[:, 0] <= ev[:, 1] + 1e-15).all() and (ev[:, 1] <= ev[:, 2] + 1e-15).all()
    assert (ev[:, 0] >= 0.01 * ev[:, 2] * (1 - 1e-9)).all()      # inflation floor (ref :311-323)


# ---------------------------------------------------------------------------------------
# C3-wide: the same scan-to-map shape on a voxel table that is NOT cache-resident
# (3.2e5 valid leaves = 26 MB of records + a 42 MB dense index grid, against C3's 1.7 MB)
# ---------------------------------------------------------------------------------------
def test_c3_wide_parity(pkg, O, S):
    cfg = S.config_c3_wide()
    prm = O.default_params(resolution=0.5, step_size=0.1, trans_epsilon=1e-4, max_iterations=35, num_threads=16)
    grid = O.Grid(cfg["target"], prm)
    assert grid.n_leaves >= 150000
    ndt = make_ndt(pkg, resolution=0.5, max_iterations=35)
    ndt.setInputTarget(cfg["target"])
    gi = ndt.getGridInfo()
    assert gi["n_leaves"] == grid.n_leaves and gi["n_leaves"] * 80 >= 12e6
    assert_leaves_match(ndt.getLeaves(), grid.export())
    ndt.setInputSource(cfg["source"])
    prm64 = O.default_params(resolution=0.5, step_size=0.1, trans_epsilon=1e-4, max_iterations=35, num_threads=16,
                             pair_mode=2)
    for T in (cfg["guess"], cfg["gt"]):
        p = O.matrix_to_pose(T)
        e = ndt.evalDerivatives(p)[0]
        assert_derivs_match(e, grid.derivatives(cfg["source"], p))
        assert_derivs_match(e, grid.derivatives(cfg["source"], p, params=prm64), 1e-9)
    T = ndt.align(cfg["guess"])
    ref = grid.align(cfg["source"], cfg["guess"], params=prm64)
    dt, dr = S.pose_error(T, ref["T"])
    assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD, (dt, dr)
    assert ndt.getResult()["iterations"] == ref["iterations"]
    assert S.pose_error(T, cfg["gt"])[0] < 0.05
    # a second, different target through the same engine (the steady-state build path that derives
    # its geometry on the device), then back: bit-identical leaves both times
    L1 = ndt.getLeaves()
    c3 = S.config_c3()
    ndt.setInputTarget(c3["target"])
    assert_leaves_match(ndt.getLeaves(), O.Grid(c3["target"], prm).export())
    ndt.setInputTarget(cfg["target"])
    L2 = ndt.getLeaves()
    for k in ("cell", "count", "mean", "cov", "icov"):
        assert np.array_equal(L1[k], L2[k]), k


def test_crowded_voxels_across_sort_and_run_tiles(pkg, O):
    """Voxels that hold thousands of points: their runs of equal cell key straddle several tiles of
    the run search (2048 keys; the carry-in run's head is found by wave 0 with 64-wide probes, more
    than one probe round beyond 4096 keys) and of the sort (8192 pairs).  Membership and counts bit
    for bit, moments to the usual tolerances, against the oracle."""
    rng = np.random.default_rng(77)
    parts = []
    # crowded voxels of awkward sizes, interleaved in input order with ordinary points
    for i, m in enumerate([10000, 4097, 4096, 2049, 8193, 6000, 2047, 12289]):
        c = np.array([3.0 * i - 10.0, 20.0, 0.0]) + 0.5
        parts.append(c + rng.uniform(-0.45, 0.45, (m, 3)))
    parts.append(rng.uniform(-6, 6, (30000, 3)))
    tgt = np.concatenate(parts)
    tgt = tgt[rng.permutation(len(tgt))].astype(np.float32)
    kw = dict(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=5, min_points_per_voxel=6)
    grid = O.Grid(tgt, O.default_params(num_threads=4, **kw))
    ndt = pkg.NormalDistributionsTransform(device_id=0, **kw)
    for rep in range(2):   # the first build waits for the geometry, the second is the optimistic one
        ndt.setInputTarget(tgt)
        L, OL = ndt.getLeaves(), grid.export()
        assert L["count"].max() >= 12289
        assert_leaves_match(L, OL)
    # a voxel of 12 289 points fits no bucket block: the two-launch build declines (BG_BUCKET), sort-based repeats it
    assert ndt.buildCounters()[1:] == (1, 0)


@pytest.mark.parametrize("n", [8191, 8192, 8193, 16384, 24577, 65536, 100003, 262144, 300000, 2097152, 2097153, 2600001])
def test_build_at_tile_boundaries_of_the_fused_passes(pkg, O, n):
    """Cloud sizes at and around multiples of the fused sort pass's 8192-pair tile (and of the run
    search's 2048-key tile), and around 256 tiles = 2 097 152 points where the 16384-pair tile takes
    over: voxel membership and counts bit for bit against the oracle, twice (waiting build,
    optimistic build), with a few non-finite points thrown in: the whole leaf set, statistics included."""
    rng = np.random.default_rng(n)
    tgt = (rng.normal(0, 1, (n, 3)) * np.array([14.0, 9.0, 1.5])).astype(np.float32)
    tgt[rng.integers(0, n, 5)] = np.nan
    kw = dict(resolution=0.7, step_size=0.1, trans_epsilon=1e-4, max_iterations=5, min_points_per_voxel=6)
    grid = O.Grid(tgt, O.default_params(num_threads=4, **kw))
    OL = grid.export()
    ndt = pkg.NormalDistributionsTransform(device_id=0, **kw)
    for rep in range(2):
        ndt.setInputTarget(tgt)
        assert_leaves_match(ndt.getLeaves(), OL)
    bc = ndt.buildCounters()
    assert bc[0] == 0
    # the second (steady-state) build of a cloud that fits goes through in two launches
    assert bc[1:] == ((0, 1) if n <= 1310720 else (0, 0)), bc


def test_one_engine_many_targets_in_turn(pkg, S):
    """One engine voxelises very different clouds one after the other (the dense index, the dirty-cell
    reset, the sort plan, the tag tables of the fused launches and the optimistic path all carry state
    from build to build): every grid equals the one a fresh engine builds, bit for bit."""
    rng = np.random.default_rng(11)
    clouds = [S.config_c1()["target"], S.config_c2()["target"], rng.uniform(-3, 3, (7, 3)).astype(np.float32),
              S.config_c3()["target"][:300000], rng.uniform(-40, 40, (50000, 3)).astype(np.float32),
              S.config_c2()["target"][:9000], S.config_c3()["target"][::3] + np.float32(250.0)]
    kw = dict(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=5)
    fresh = []
    for c in clouds:
        e = pkg.NormalDistributionsTransform(device_id=0, **kw)
        try:
            e.setInputTarget(c); fresh.append(e.getLeaves())
        except pkg.NdtError:
            fresh.append(None)
    ndt = pkg.NormalDistributionsTransform(device_id=0, **kw)
    order = [0, 3, 2, 1, 4, 6, 5, 3, 3, 0, 2, 6, 1, 4, 5, 0]
    for k in order:
        if fresh[k] is None:
            with pytest.raises(pkg.NdtError):
                ndt.setInputTarget(clouds[k])
            continue
        ndt.setInputTarget(clouds[k])
        L = ndt.getLeaves()
        for f in ("cell", "count", "mean", "cov", "icov", "evals"):
            assert np.array_equal(L[f], fresh[k][f]), (k, f)
    bc = ndt.buildCounters()
    # fresh engines build sort-based (first build), this one mostly in two launches: bit-identical leaves
    assert bc[0] == 0 and bc[2] >= 8, bc


def test_two_launch_build_declines_and_the_sort_based_build_repeats_it(pkg, O):
    """The steady-state build in two launches declines what it cannot hold, and the sort-based pipeline repeats the
    build with the same leaves as a first (sort-based) build of that cloud, bit for bit:
      * a cloud of isolated points -- more distinct cells in a bucket than its LDS hash table takes: the bucket notices
        AFTER other buckets have published leaves (BG_BUCKET from the last block; the host clears the whole grid);
      * coordinates beyond 2^23 voxels -- floor(p / leaf) - min_b stops being exact in f32 there, one voxel could
        straddle two buckets: declined before anything is written."""
    rng = np.random.default_rng(31)
    kw = dict(resolution=0.5, step_size=0.1, trans_epsilon=1e-4, max_iterations=5, min_points_per_voxel=6)
    # (a) 1.1 M points, almost every one alone in its voxel, plus a few hundred real leaves
    sparse = rng.uniform(-150.0, 150.0, (1100000, 3)) * np.array([1.0, 1.0, 0.2])
    dense = np.concatenate([c + rng.uniform(-0.2, 0.2, (40, 3)) for c in rng.uniform(-100.0, 100.0, (300, 3))])
    tgt = np.concatenate([sparse, dense])[rng.permutation(1100000 + 300 * 40)].astype(np.float32)
    grid = O.Grid(tgt, O.default_params(num_threads=8, **kw))
    OL = grid.export()
    ndt = pkg.NormalDistributionsTransform(device_id=0, **kw)
    first = None
    for rep in range(3):
        ndt.setInputTarget(tgt)
        L = ndt.getLeaves()
        assert np.array_equal(L["cell"], OL["cell"]) and np.array_equal(L["count"], OL["count"]) and len(L["cell"]) >= 250
        np.testing.assert_allclose(L["mean"], OL["mean"], rtol=1e-12, atol=0)
        if first is None:
            first = L
        for f in ("mean", "cov", "icov", "evals"):
            assert np.array_equal(L[f], first[f]), (rep, f)
    assert ndt.buildCounters()[1:] == (1, 0)   # declined once, then not tried again for the next 8 builds; never built in two launches
    # (b) the same engine, an ordinary cloud 6 000 km from the origin
    far = (rng.normal(0, 1, (60000, 3)) * np.array([8.0, 6.0, 1.0]) + np.array([6.0e6, 0.0, 0.0])).astype(np.float32)
    fresh = pkg.NormalDistributionsTransform(device_id=0, **kw)
    fresh.setInputTarget(far)
    want = fresh.getLeaves()
    assert len(want["cell"]) > 10
    ndt2 = pkg.NormalDistributionsTransform(device_id=0, **kw)
    for rep in range(3):
        ndt2.setInputTarget(far)
        L = ndt2.getLeaves()
        for f in ("cell", "count", "mean", "cov", "icov", "evals"):
            assert np.array_equal(L[f], want[f]), (rep, f)
    bc = ndt2.buildCounters()
    assert bc[1] == 1 and bc[2] == 0, bc       # the first steady-state build declined, the next went sort-based straight away
