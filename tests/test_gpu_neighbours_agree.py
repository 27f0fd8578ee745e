"""The four evaluators and the reference pair a point with the same voxels where the classification is delicate.
ndt_score_points, ndt_eval_derivatives, the continuous-time evaluation and the D2D evaluation all find a moved point's
neighbours through csrc/ndt_neighbors_device.h; here every one of them is counted against the CPU oracle on points that lie
ON voxel faces, edges and corners.
Target: leaf 1.0, the voxels [0,4) x [0,3) x [0,3) minus the interior voxel (1, 1, 1), 8 points each at the centre +- 0.25
per axis.  Source: the f32-exact lattice of spacing 0.5 over [-1.5, 5.5] x [-1.5, 4.5] x [-1.5, 4.5] (15 x 13 x 13 = 2535
points: p == lo is inside, p == hi outside, points more than a leaf outside; ten blocks of 256, the last one ragged) plus
one NaN point and one at 1e30.  Pose: the identity, where the f32 move, CT's f64 chain and D2D's f64 move all return
the input exactly.  Every assertion is an integer equality."""
import numpy as np
import pytest

from test_d2d_cpu import d2d_pairs

LEAF = 1.0
HOLE = (1, 1, 1)
ZERO6 = np.zeros(6)


def target_cloud():
    corners = np.array([[sx, sy, sz] for sx in (-0.25, 0.25) for sy in (-0.25, 0.25) for sz in (-0.25, 0.25)])
    vox = [(i, j, k) for i in range(4) for j in range(3) for k in range(3) if (i, j, k) != HOLE]
    return np.concatenate([np.array(v) + 0.5 + corners for v in vox]).astype(np.float32)


def lattice():
    ax = [np.arange(lo, hi + 0.25, 0.5) for lo, hi in ((-1.5, 5.5), (-1.5, 4.5), (-1.5, 4.5))]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    assert len(g) == 15 * 13 * 13
    return g


def source_cloud():
    return np.concatenate([lattice(), np.array([[np.nan, 1.0, 1.0], [1e30, 1e30, 1e30]], np.float32)])


def oracle_counts(O, method):
    """neighbours per source point by the reference's own lookup.  The two special points are not handed to it: the
    reference skips a point that is not finite before any lookup (svn_ndt_impl.hpp:573), and the one at 1e30 lies more
    than a leaf outside the grid on every axis, where no neighbourhood of any method reaches a voxel."""
    grid = O.Grid(target_cloud(), O.default_params(resolution=LEAF))
    n = np.array([len(grid.neighbors(p, method)) for p in lattice()], np.int64)
    return grid, np.concatenate([n, [0, 0]])


def pairs_counts(points, leaves, grid_info, method):
    pi, _ = d2d_pairs(points, leaves, grid_info, method)
    return np.bincount(pi, minlength=len(points)).astype(np.int64)


def test_inputs_oracle_and_numpy_rule_agree_on_the_lattice(O):
    """no GPU: the reference's lookup and the NumPy restatement of the rule count the same neighbours for every lattice
    point, so the expectation the GPU tests use does not depend on which of the two is asked"""
    for name, method in (("DIRECT1", O.DIRECT1), ("DIRECT7", O.DIRECT7)):
        grid, want = oracle_counts(O, method)
        info = dict(min_b=grid.min_b, max_b=grid.max_b, div_b=grid.div_b, leaf_size=float(grid.info.leaf))
        got = pairs_counts(source_cloud(), grid.export(), info, name)
        assert np.array_equal(got, want), name
        # 35 voxels with 2 x 2 x 2 lattice points each; the one voxel with six neighbours, (2, 1, 1), has the hole beside it
        if name == "DIRECT1":
            assert (want > 0).sum() == 35 * 8 and want.max() == 1
        else:
            assert (want > 0).sum() > 35 * 8 and want.max() == 6


@pytest.fixture(scope="module")
def rig(pkg, O):
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=LEAF)
    ndt.setInputTarget(target_cloud())
    src = source_cloud()
    ndt.setInputSource(src)
    assert pkg.setSourceTimes(ndt, np.linspace(0.0, 1.0, len(src)).astype(np.float32)) == len(src)
    # D2D: one record per lattice point, the moments of 8 points at the point +- 2^-3 per axis (sums and mean exact)
    p = lattice().astype(np.float64)
    h2 = 8 * 0.125 ** 2
    mom = np.stack([8 * p[:, 0], 8 * p[:, 1], 8 * p[:, 2], 8 * p[:, 0] ** 2 + h2, 8 * p[:, 0] * p[:, 1], 8 * p[:, 0] * p[:, 2],
                    8 * p[:, 1] ** 2 + h2, 8 * p[:, 1] * p[:, 2], 8 * p[:, 2] ** 2 + h2], axis=1)
    assert pkg.setSourceDistributions(ndt, count=np.full(len(p), 8, np.int32), moments=mom) == (len(p), len(p))
    assert np.array_equal(pkg.getSourceDistributions(ndt)["mean"], p)
    want = {name: oracle_counts(O, getattr(O, name))[1] for name in ("DIRECT1", "DIRECT7", "KDTREE", "DIRECT26")}
    return dict(ndt=ndt, src=src, want=want)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True], ids=["f64", "packed48"])
@pytest.mark.parametrize("method", ["DIRECT1", "DIRECT7"])
def test_every_evaluator_counts_the_references_pairs(pkg, rig, method, packed):
    ndt, want = rig["ndt"], rig["want"][method]
    ndt.setNeighborhoodSearchMethod(getattr(pkg, method))
    ndt.setRecordFormat(pkg.RECORDS_PACKED48 if packed else pkg.RECORDS_F64)
    try:
        # the expectation from the engine's own grid is the reference's
        assert np.array_equal(pairs_counts(rig["src"], ndt.getLeaves(), ndt.getGridInfo(), method), want)
        n_nb = ndt.scorePoints(np.eye(4), fields=["n_neighbors"])["n_neighbors"]
        assert np.array_equal(n_nb.astype(np.int64), want)
        pairs, with_nb = int(want.sum()), int((want > 0).sum())
        ev = ndt.evalDerivatives(ZERO6)[0]
        assert (ev["n_pairs"], ev["n_with_neighbors"]) == (pairs, with_nb)
        ct = pkg.evalDerivativesCT(ndt, ZERO6, ZERO6)[0]
        assert (ct["n_pairs"], ct["n_with_neighbors"]) == (pairs, with_nb)
        # D2D's source is the lattice alone: neither special point has a neighbour
        d2d = pkg.evalDerivativesD2D(ndt, ZERO6)[0]
        assert (d2d["n_pairs"], d2d["n_with_neighbors"]) == (pairs, with_nb)
    finally:
        ndt.setRecordFormat(pkg.RECORDS_F64)
        ndt.setNeighborhoodSearchMethod(pkg.DIRECT7)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["KDTREE", "DIRECT26"])
def test_27_cell_neighbourhoods_count_the_references_pairs(pkg, rig, method):
    ndt, want = rig["ndt"], rig["want"][method]
    ndt.setNeighborhoodSearchMethod(getattr(pkg, method))
    try:
        n_nb = ndt.scorePoints(np.eye(4), fields=["n_neighbors"])["n_neighbors"].astype(np.int64)
        ev = ndt.evalDerivatives(ZERO6)[0]
        assert int(n_nb.sum()) == ev["n_pairs"] == int(want.sum())
        assert int((n_nb > 0).sum()) == ev["n_with_neighbors"] == int((want > 0).sum())
    finally:
        ndt.setNeighborhoodSearchMethod(pkg.DIRECT7)
