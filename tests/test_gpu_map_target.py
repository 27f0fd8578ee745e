"""The voxel map's per-voxel moments (ndt_map_enable_moments) and the NDT target made from them
(ndt_set_target_from_map_moments), against
  (A) the oracle on the concatenation of everything added, or on the stated subset of it, and
  (B) moments_numpy (tests/test_map_target_cpu.py): f64 sums per voxel in input order -- which that file shows to be the
      oracle's own intermediate state, bit for bit.
Moments are compared with np.array_equal.  Leaves, evaluations and aligns are held to the tolerances of
tests/test_gpu_parity.py: cells, counts and geometry exact; mean 1e-12 relative; covariance / inverse 1e-9 / 1e-7 of the
matrix's largest entry (1e-6 / 1e-4 at +3 km, that file's cap for the placement); score and NVTL 1e-9; gradient / Hessian
1e-9 of their norms against the oracle's f64 evaluation; final transform within 1 mm / 0.1 mrad.
Base shape: 4 scans of 32 x 256 beams (32 768 points), each moved by its pose."""
import ctypes as C

import numpy as np
import pytest

from test_map_target_cpu import host_transform_f64, moments_numpy, voxel_ijk

pytestmark = pytest.mark.gpu

ALIGN_TOL_M, ALIGN_TOL_RAD = 1e-3, 1e-4
INVALID_ARG, NO_TARGET, GRID_OVERFLOW, UNSUPPORTED = -1, -4, -6, -9
KW = dict(step_size=0.1, trans_epsilon=1e-4, max_iterations=35)


def engine(pkg, leaf=1.0, **kw):
    p = dict(KW, resolution=leaf)
    p.update(kw)
    return pkg.NormalDistributionsTransform(device_id=0, **p)


def oracle_params(O, leaf=1.0, **kw):
    return O.default_params(resolution=leaf, num_threads=8, **dict(KW, **kw))


def assert_leaves_match(L, OL, cov_rtol=1e-9, label=""):
    assert len(OL["cell"]) > 0
    assert np.array_equal(L["cell"], OL["cell"])
    assert np.array_equal(L["count"], OL["count"])
    worst = {}
    for k in ("cov", "icov"):
        scale = np.abs(OL[k]).max(axis=(1, 2), keepdims=True)
        worst[k] = float((np.abs(L[k] - OL[k]) / scale).max())
    scale = np.abs(OL["evals"]).max(axis=1, keepdims=True)
    worst["evals"] = float((np.abs(L["evals"] - OL["evals"]) / scale).max())
    worst["mean"] = float((np.abs(L["mean"] - OL["mean"]) / np.abs(OL["mean"])).max())
    print("leaves %s: %d leaves, worst relative error %s" % (label, len(OL["cell"]), worst))
    np.testing.assert_allclose(L["mean"], OL["mean"], rtol=1e-12, atol=0)
    assert worst["cov"] < cov_rtol and worst["icov"] < 100 * cov_rtol and worst["evals"] < 100 * cov_rtol, worst


def assert_grid_matches(gi, grid, n_points):
    assert np.array_equal(gi["min_b"], grid.min_b) and np.array_equal(gi["max_b"], grid.max_b)
    assert np.array_equal(gi["div_b"], grid.div_b)
    assert gi["n_cells"] == int(np.prod(grid.div_b.astype(np.int64))) and gi["n_leaves"] == grid.n_leaves
    assert gi["n_target_points"] == n_points


def assert_derivs_match(e, d, tol=1e-9):
    assert e["n_pairs"] == d["n_pairs"] and e["n_with_neighbors"] == d["n_with_neighbors"]
    assert e["score"] == pytest.approx(d["score"], rel=1e-9, abs=1e-9)
    assert e["nvtl_sum"] == pytest.approx(d["nvtl_sum"], rel=1e-9, abs=1e-9)
    gn, hn = np.linalg.norm(d["gradient"]), np.linalg.norm(d["hessian"])
    assert np.linalg.norm(e["gradient"] - d["gradient"]) <= tol * gn + 1e-12
    assert np.linalg.norm(e["hessian"] - d["hessian"]) <= tol * hn + 1e-12


def leaf_bytes(pkg, ndt):
    """ndt_export_leaves as the bytes it writes."""
    n = int(ndt.getGridInfo()["n_leaves"])
    buf = (pkg.Leaf * max(n, 1))()
    assert pkg.lib().ndt_export_leaves(ndt._h, buf, n) == n
    return bytes(buf)[:n * C.sizeof(pkg.Leaf)]


def eval_words(pkg, ndt, pose6):
    """the 32 words of one evaluation, as bits"""
    p = np.ascontiguousarray(pose6, np.float64).reshape(1, 6)
    out = np.zeros((1, 32))
    assert pkg.lib().ndt_eval_derivatives(ndt._h, p.ctypes.data_as(C.POINTER(C.c_double)), None, 1, 1,
                                          out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return out.view(np.uint64).copy()


def moments_map(pkg, leaf, pieces, poses=None, capacity=0, moments=True, **kw):
    ndt = engine(pkg, leaf, **kw)
    ndt.mapReset(leaf, initial_capacity=capacity)
    if moments:
        ndt.mapEnableMoments()
    for k, piece in enumerate(pieces):
        ndt.mapAdd(piece, pose=None if poses is None else poses[k])
    return ndt


def code_of(pkg, fn, *a, **k):
    with pytest.raises(pkg.NdtError) as ei:
        fn(*a, **k)
    return ei.value.code


@pytest.fixture(scope="module")
def base():
    from slam_sam_amd import replay
    stream = replay.make_stream(n_frames=4, beams=32, cols=256)
    scans = [np.ascontiguousarray(s[:, :3], np.float32) for s, _ in stream]
    poses = [T for _, T in stream]
    moved = [host_transform_f64(T, s) for s, T in zip(scans, poses)]
    cat = np.concatenate(moved)
    assert len(cat) == 32768
    return dict(scans=scans, poses=poses, moved=moved, cat=cat)


_grids = {}


def oracle_grid(O, key, cloud, leaf, **kw):
    """one oracle grid per case, shared by the tests that need it"""
    if key not in _grids:
        prm = oracle_params(O, leaf, **kw)
        g = O.Grid(cloud, prm)
        _grids[key] = (g, g.export(), prm)
    return _grids[key]


# ---- 1. moments are the sequential sums, bit for bit -------------------------------------------------------------------
def moment_cases(base, name):
    """(pieces, poses or None, initial capacity, the concatenation as the map sees it)"""
    cat = base["cat"]
    if name == "poses":
        return base["scans"], base["poses"], 0, cat
    if name == "ragged":
        cuts = np.r_[0, np.cumsum([1, 0, 63, 4097, 257, 1, 9000]), len(cat)]
        return [cat[a:b] for a, b in zip(cuts[:-1], cuts[1:])], None, 0, cat
    if name == "grown":
        return base["moved"], None, 64, cat
    if name == "crowded":
        rng = np.random.default_rng(5)
        crowd = rng.uniform(0.05, 0.95, (5000, 3)).astype(np.float32) + np.float32([3, -2, 1])
        other = rng.uniform(-6, 6, (700, 3)).astype(np.float32)
        pts = np.concatenate([crowd[:2000], other[:300], crowd[2000:2001], crowd[2001:], other[300:]])
        cuts = [0, 2300, 2301, len(pts)]
        return [pts[a:b] for a, b in zip(cuts[:-1], cuts[1:])], None, 0, pts
    if name == "nonfinite":
        rng = np.random.default_rng(9)
        bad = cat.copy()
        at = rng.choice(len(bad), 300, replace=False)
        bad[at[:100], 0] = np.nan
        bad[at[100:200], 1] = np.inf
        bad[at[200:], 2] = -np.inf
        return np.array_split(bad, 4), None, 0, bad
    raise KeyError(name)


@pytest.mark.parametrize("name", ["poses", "ragged", "grown", "crowded", "nonfinite"])
def test_moments_are_the_sequential_sums_bit_for_bit(pkg, base, name):
    leaf = 1.0
    pieces, poses, cap, seen = moment_cases(base, name)
    ndt = moments_map(pkg, leaf, pieces, poses, cap)
    assert ndt.mapHasMoments()
    ijk, count, sums = ndt.mapExportMoments()
    bijk, bcount, bsums = moments_numpy(seen, leaf)
    assert ijk.dtype == np.int32 and count.dtype == np.int32 and sums.dtype == np.float64
    assert np.array_equal(ijk, bijk) and np.array_equal(count, bcount)
    assert np.array_equal(sums, bsums)                                            # the bits of all nine sums
    info = ndt.mapInfo()
    fin = np.isfinite(seen).all(axis=1)
    assert info["n_points"] == int(fin.sum()) == int(count.sum()) and info["n_points_dropped"] == int((~fin).sum())
    if name == "grown":
        assert info["n_grows"] >= 1 and info["capacity"] >= 2 * len(count)
    if name == "crowded":
        assert int(count.max()) == 5000
    if name == "poses":
        assert len(count) == 4760 and int(count.max()) == 179
    # ijk and counts are those of the centroid export; min_points filters as it does there
    xyz, xcnt = ndt.mapExport(with_counts=True)
    assert np.array_equal(xcnt, count) and np.array_equal(voxel_ijk(xyz, leaf), ijk)
    keep = bcount >= 5
    fijk, fcount, fsums = ndt.mapExportMoments(min_points=5)
    assert np.array_equal(fijk, bijk[keep]) and np.array_equal(fcount, bcount[keep]) and np.array_equal(fsums, bsums[keep])
    # ... and the float side of the map does not notice the moments
    plain = moments_map(pkg, leaf, pieces, poses, cap, moments=False)
    assert not plain.mapHasMoments()
    pxyz, pcnt = plain.mapExport(with_counts=True)
    assert np.array_equal(pxyz.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(pcnt, xcnt)


# ---- 2. whole-map target against the oracle on the concatenation -------------------------------------------------------
WHOLE = {
    "leaf1.0": (1.0, 0.0, {}, 1e-9),
    "leaf0.5": (0.5, 0.0, {}, 1e-9),
    "cov_mode1": (1.0, 0.0, dict(cov_mode=1), 1e-9),
    "min_points6": (1.0, 0.0, dict(min_points_per_voxel=6), 1e-9),
    "shift3km": (1.0, 3000.0, {}, 1e-6),     # the project's cap for that placement (test_gpu_parity.py)
}


@pytest.mark.parametrize("name", list(WHOLE))
def test_whole_map_target_equals_the_oracle_on_the_concatenation(pkg, O, base, name):
    leaf, shift, kw, cov_rtol = WHOLE[name]
    moved = base["moved"]
    if shift:
        moved = [(m.astype(np.float64) + [shift, 0.0, 0.0]).astype(np.float32) for m in moved]
    cat = np.concatenate(moved)
    grid, OL, _ = oracle_grid(O, name, cat, leaf, **kw)
    if name in ("leaf1.0", "leaf0.5"):
        assert grid.n_leaves == {1.0: 919, 0.5: 1161}[leaf]
    ndt = moments_map(pkg, leaf, moved, **kw)
    ndt.setInputTargetFromMapMoments()
    assert_grid_matches(ndt.getGridInfo(), grid, len(cat))
    L = ndt.getLeaves()
    assert_leaves_match(L, OL, cov_rtol, "moments target vs oracle [%s]" % name)
    # the same against the ordinary build of the concatenation on a second handle
    ref = engine(pkg, leaf, **kw)
    ref.setInputTarget(cat)
    gi, gr = ndt.getGridInfo(), ref.getGridInfo()
    for k in ("min_b", "max_b", "div_b"):
        assert np.array_equal(gi[k], gr[k])
    assert gi["n_cells"] == gr["n_cells"] and gi["n_leaves"] == gr["n_leaves"] and gi["n_target_points"] == gr["n_target_points"]
    assert_leaves_match(L, ref.getLeaves(), cov_rtol, "moments target vs setInputTarget [%s]" % name)


# ---- 3. evaluation and align --------------------------------------------------------------------------------------------
def test_evaluation_and_align_on_the_moments_target(pkg, O, S, base):
    leaf = 1.0
    cat, src, T_gt = base["cat"], base["scans"][3], base["poses"][3]
    grid, _, _ = oracle_grid(O, "leaf1.0", cat, leaf)
    prm64 = oracle_params(O, leaf, pair_mode=2)          # the reference's formulas with f64 products
    ndt = moments_map(pkg, leaf, base["moved"])
    ndt.setInputTargetFromMapMoments()
    ndt.setInputSource(src)
    p_gt = O.matrix_to_pose(T_gt)
    p_off = p_gt + [0.05, -0.03, 0.02, 0.01, -0.005, 0.008]
    for p, e in zip((p_gt, p_off), ndt.evalDerivatives(np.stack([p_gt, p_off]))):
        assert_derivs_match(e, grid.derivatives(src, p, params=prm64), 1e-9)
    guess = O.pose_to_matrix(p_off)
    T = ndt.align(guess)
    ref = engine(pkg, leaf)
    ref.setInputTarget(cat)
    ref.setInputSource(src)
    T_ref = ref.align(guess)
    dt, dr = S.pose_error(T, T_ref)
    print("align on the moments target vs setInputTarget(concatenation): %.3e m %.3e rad" % (dt, dr))
    assert ndt.getResult()["converged"] and dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD, (dt, dr)


# ---- 4. box ---------------------------------------------------------------------------------------------------------------
def in_box(pts, leaf, box_min, box_max):
    """the points whose voxel is inside the box: the same f32 floor on both sides"""
    ijk = voxel_ijk(pts, leaf)
    lo = voxel_ijk(np.float32(box_min)[None], leaf)[0]
    hi = voxel_ijk(np.float32(box_max)[None], leaf)[0]
    return ((ijk >= lo) & (ijk <= hi)).all(axis=1)


def assert_box_equals_oracle(pkg, O, ndt, cloud, leaf, box_min, box_max, label):
    sub = cloud[in_box(cloud, leaf, box_min, box_max)]
    assert 0 < len(sub) < len(cloud)
    grid = O.Grid(sub, oracle_params(O, leaf))
    ndt.setInputTargetFromMapMoments(box_min, box_max)
    assert_grid_matches(ndt.getGridInfo(), grid, len(sub))
    assert_leaves_match(ndt.getLeaves(), grid.export(), 1e-9, label)
    return sub


def test_box_around_the_vehicle(pkg, O, base):
    leaf = 1.0
    cat = base["cat"]
    ndt = moments_map(pkg, leaf, base["moved"])
    c = base["poses"][3][:3, 3]
    assert_box_equals_oracle(pkg, O, ndt, cat, leaf, c - [12.0, 9.0, 4.0], c + [12.0, 9.0, 4.0], "box around the last pose")
    # a box whose geometry is fixed by occupied voxels below min_points_per_voxel: an occupied voxel with fewer than three
    # points as the box's upper corner, the voxel 20 x 20 x 10 below it as the lower one -- the first such box that holds
    # well-filled voxels too and in which the bounds of all occupied voxels differ from the bounds of those with three
    # points or more
    ijk, count, _ = moments_numpy(cat, leaf)
    found = None
    for v in ijk[count < 3][::-1]:
        lo = v - [20, 20, 10]
        inside = ((ijk >= lo) & (ijk <= v)).all(axis=1)
        cand = inside & (count >= 3)
        if (count[cand] >= 10).sum() >= 3 and (not np.array_equal(ijk[inside].min(0), ijk[cand].min(0)) or
                                not np.array_equal(ijk[inside].max(0), ijk[cand].max(0))):
            found = (lo, v)
            break
    assert found is not None
    lo, hi = found
    assert_box_equals_oracle(pkg, O, ndt, cat, leaf, (lo + 0.5) * leaf, (hi + 0.5) * leaf, "box with sparse border voxels")


def test_two_patches_30_km_apart(pkg, O, base):
    leaf = 0.5
    far = np.float64([21213.25, 21213.25, 0.0])                                   # 30 km along the diagonal
    a = base["moved"][0]
    b = (base["moved"][1].astype(np.float64) + far).astype(np.float32)
    both = np.concatenate([a, b])
    ext = voxel_ijk(both, leaf)
    assert np.prod((ext.max(0) - ext.min(0) + 1).astype(np.float64)) >= 2**31 - 1   # the whole map exceeds a dense index
    ndt = moments_map(pkg, leaf, [a, b])
    ndt.setInputSource(base["scans"][0])
    p0 = O.matrix_to_pose(base["poses"][0])
    margin = np.float32([1.0, 1.0, 1.0])
    assert_box_equals_oracle(pkg, O, ndt, both, leaf, a.min(0) - margin, a.max(0) + margin, "patch A")
    leaves, words = leaf_bytes(pkg, ndt), eval_words(pkg, ndt, p0)
    # the whole map is refused, and so is an empty box: the target stays exactly as it was
    assert code_of(pkg, ndt.setInputTargetFromMapMoments) == GRID_OVERFLOW
    assert leaf_bytes(pkg, ndt) == leaves and np.array_equal(eval_words(pkg, ndt, p0), words)
    assert code_of(pkg, ndt.setInputTargetFromMapMoments, [5000.0, 5000.0, 0.0], [5010.0, 5010.0, 10.0]) == NO_TARGET
    assert code_of(pkg, ndt.setInputTargetFromMapMoments, [10.0, 10.0, 10.0], [-10.0, -10.0, -10.0]) == NO_TARGET
    assert leaf_bytes(pkg, ndt) == leaves and np.array_equal(eval_words(pkg, ndt, p0), words)
    assert_box_equals_oracle(pkg, O, ndt, both, leaf, b.min(0) - margin, b.max(0) + margin, "patch B")


# ---- 5. determinism -------------------------------------------------------------------------------------------------------
def test_two_handles_hold_the_same_table(pkg, O, base):
    leaf = 1.0
    small = moments_map(pkg, leaf, base["scans"], base["poses"], capacity=64)
    large = moments_map(pkg, leaf, base["scans"], base["poses"], capacity=0)
    assert small.mapInfo()["n_grows"] >= 1 and large.mapInfo()["n_grows"] == 0
    p = O.matrix_to_pose(base["poses"][3]) + [0.05, -0.03, 0.02, 0.01, -0.005, 0.008]
    out = []
    for ndt in (small, large):
        ndt.setInputTargetFromMapMoments()
        ndt.setInputSource(base["scans"][3])
        out.append((leaf_bytes(pkg, ndt), eval_words(pkg, ndt, p)))
    assert out[0][0] == out[1][0] and len(out[0][0]) > 0
    assert np.array_equal(out[0][1], out[1][1])


# ---- 6. state and refusals ------------------------------------------------------------------------------------------------
def test_refusals(pkg, base):
    ndt = engine(pkg, 1.0)
    assert not ndt.mapHasMoments()
    assert code_of(pkg, ndt.mapEnableMoments) == INVALID_ARG                      # no map
    assert code_of(pkg, ndt.setInputTargetFromMapMoments) == INVALID_ARG
    assert code_of(pkg, ndt.mapExportMoments) == INVALID_ARG
    ndt.mapReset(1.0)
    assert code_of(pkg, ndt.mapExportMoments) == INVALID_ARG                      # a map without moments
    assert code_of(pkg, ndt.setInputTargetFromMapMoments) == INVALID_ARG
    ndt.mapAdd(base["moved"][0])
    assert code_of(pkg, ndt.mapEnableMoments) == INVALID_ARG                      # the map holds points already
    assert code_of(pkg, ndt.setInputTargetFromMapMoments) == INVALID_ARG and not ndt.mapHasMoments()
    ndt.mapReset(1.0)
    ndt.mapEnableMoments()
    assert code_of(pkg, ndt.mapEnableMoments) == INVALID_ARG                      # twice
    assert ndt.mapHasMoments()
    assert code_of(pkg, ndt.setInputTargetFromMapMoments) == NO_TARGET            # an empty map
    ndt.mapReset(1.0)
    assert not ndt.mapHasMoments()                                                # a new map starts without
    half = moments_map(pkg, 0.5, base["moved"][:1], resolution=1.0)               # leaf != resolution
    assert code_of(pkg, half.setInputTargetFromMapMoments) == INVALID_ARG


def test_state_after_a_moments_target(pkg, O, base):
    leaf = 1.0
    cat = base["cat"]
    ndt = moments_map(pkg, leaf, base["moved"])
    ndt.setInputTargetFromMapMoments()
    ndt.setInputSource(base["scans"][3])
    guess = base["poses"][3]
    ndt.align(guess)
    assert code_of(pkg, ndt.getFitnessScore) == UNSUPPORTED                       # no target points are retained
    ndt.setParams(eig_inflation_ratio=0.05)                                       # the grid cannot be re-voxelised ...
    assert code_of(pkg, ndt.align, guess) == NO_TARGET
    ndt.setInputTargetFromMapMoments()                                            # ... but the map is still there
    grid, OL, _ = oracle_grid(O, "eig0.05", cat, leaf, eig_inflation_ratio=0.05)
    assert_grid_matches(ndt.getGridInfo(), grid, len(cat))
    assert_leaves_match(ndt.getLeaves(), OL, 1e-9, "after a new eig_inflation_ratio")
    ndt.align(guess)
    assert ndt.getResult()["converged"]


def test_map_calls_leave_the_rest_of_the_handle_alone(pkg, base):
    leaf = 1.0
    ndt = engine(pkg, leaf)
    ndt.setInputTarget(base["cat"])
    ndt.setInputSource(base["scans"][3])
    ndt.putKeyframe(7, base["scans"][0])
    T = ndt.align(base["poses"][3])

    def state():
        h = ndt.getIterationHistory()
        return (leaf_bytes(pkg, ndt), ndt.sourceSize(), [a.tobytes() for a in h], ndt.getTiming()["n_eval_launches"],
                ndt.keyframeCount(), ndt.getFinalTransformation().tobytes())

    before = state()
    ndt.mapReset(leaf)
    ndt.mapEnableMoments()
    for m in base["moved"]:
        ndt.mapAdd(m)
    ndt.mapExportMoments()
    assert ndt.mapHasMoments()
    assert state() == before
    assert np.array_equal(ndt.align(base["poses"][3]), T)


def test_centroid_target_from_a_map_with_moments_is_unchanged(pkg, base):
    leaf = 0.25                                            # (centroids of 0.25 m voxels into 1 m leaves)
    out = []
    for moments in (True, False):
        ndt = engine(pkg, 1.0)
        ndt.mapReset(leaf)
        if moments:
            ndt.mapEnableMoments()
        for m in base["moved"]:
            ndt.mapAdd(m)
        ndt.setInputTargetFromMap(1)
        gi = ndt.getGridInfo()
        out.append((leaf_bytes(pkg, ndt), gi["n_cells"], gi["n_target_points"]))
        assert gi["n_leaves"] > 0
    assert out[0] == out[1]


def test_hand_over_between_the_ordinary_build_and_the_moments_target(pkg, O, base):
    """One handle goes ordinary target -> moments target -> ordinary target -> boxed moments target -> ... : each build kind
    has to reset the dense index cells the other one published.  A stale cell would show as a leaf or a pair too many, so
    cells, counts and pair counts are compared exactly with fresh handles that built only that target; the moments
    targets, which are deterministic, byte for byte."""
    leaf = 1.0
    cat, src = base["cat"], base["scans"][3]
    other = (base["moved"][1].astype(np.float64) + [7.3, -4.1, 0.6]).astype(np.float32)      # other cells, another extent
    p = O.matrix_to_pose(base["poses"][3]) + [0.05, -0.03, 0.02, 0.01, -0.005, 0.008]
    c = base["poses"][3][:3, 3]
    box = (c - [12.0, 9.0, 4.0], c + [12.0, 9.0, 4.0])

    def fresh(setup):
        f = moments_map(pkg, leaf, base["moved"])
        setup(f)
        f.setInputSource(src)
        return f.getLeaves(), leaf_bytes(pkg, f), f.evalDerivatives(p)[0], eval_words(pkg, f, p)

    want = {
        "ordinary other": fresh(lambda f: f.setInputTarget(other)),
        "ordinary cat": fresh(lambda f: f.setInputTarget(cat)),
        "moments": fresh(lambda f: f.setInputTargetFromMapMoments()),
        "moments box": fresh(lambda f: f.setInputTargetFromMapMoments(*box)),
    }
    ndt = moments_map(pkg, leaf, base["moved"])
    ndt.setInputSource(src)
    steps = ["ordinary other", "moments", "ordinary other", "moments box", "ordinary cat", "moments", "moments box",
             "ordinary other"]
    for step in steps:
        if step == "ordinary other":
            ndt.setInputTarget(other)
        elif step == "ordinary cat":
            ndt.setInputTarget(cat)
        elif step == "moments":
            ndt.setInputTargetFromMapMoments()
        else:
            ndt.setInputTargetFromMapMoments(*box)
        L, raw, e, words = ndt.getLeaves(), leaf_bytes(pkg, ndt), ndt.evalDerivatives(p)[0], eval_words(pkg, ndt, p)
        WL, wraw, we, wwords = want[step]
        assert np.array_equal(L["cell"], WL["cell"]) and np.array_equal(L["count"], WL["count"]), step
        assert e["n_pairs"] == we["n_pairs"] and e["n_with_neighbors"] == we["n_with_neighbors"], step
        assert e["score"] == pytest.approx(we["score"], rel=1e-9, abs=1e-9), step
        if step.startswith("moments"):
            assert raw == wraw and np.array_equal(words, wwords), step
        else:
            assert_leaves_match(L, WL, 1e-9, "hand-over: " + step)


def test_cpp_adapter(pkg, tmp_path):
    """tests/cpp/test_map_target.cpp against the API mocks, built with the g++ line tests/cpp/Makefile uses for them."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "tests", "cpp")
    exe = str(tmp_path / "test_map_target")
    lib = os.path.join(root, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(root, "include", "compat"), "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(d, "test_map_target.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "map target: PASS" in p.stdout
