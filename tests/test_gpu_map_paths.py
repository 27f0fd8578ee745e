"""The map side of the engine at its edges: the multi-grid union (point_pairs_kd<MODE, RADIUS, CHAIN>, its 27-entry
listing and the wave-wide fall-back to the chain walk), the keyframe archive with k_transform_append, and the voxel
downsample (k_voxel_centroids and the radix pass counts its geometry picks).

References, none of them new: the union is the SUM over its grids of the oracle's KDTREE evaluation (score rel 1e-8,
gradient / Hessian 1e-9 of the norm against pair_mode=2 and the `1.01 * rg` form against the reference arithmetic, as
tests/test_gpu_multigrid.py; per point 1e-9 as tests/test_gpu_point_scores.py; leaves as tests/test_gpu_random.py);
the window assembly is host_transform_f64, bit for bit; the downsample is voxelgrid_numpy, exact.

The unmarked tests at the top pin, on the CPU, the properties the GPU cases rely on (where the 27-leaf limit falls,
that an f32 transform or an f64 centroid sum would be told apart, which radix pass counts are reached)."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_downsample import voxelgrid_numpy
from test_gpu_keyframes import host_transform_f64
from test_gpu_random import cov_loss

gpu = pytest.mark.gpu

KW = dict(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=35)
KD_CELLS = 27          # ndt_derivs.hip: the listing holds at most this many leaves per lane
ORACLE_THREADS = 16


# ------------------------------------------------------------------------------------------------ shared helpers
def oprm(O, kw, **more):
    return O.default_params(num_threads=ORACLE_THREADS, **dict(kw, **more))


def f32_transform(T, pts):
    """The evaluation's point transform: x' = r0 x + (r1 y + (r2 z + t)) in f32, never fused."""
    T = np.asarray(T, np.float32)
    p = np.asarray(pts, np.float32)
    return np.stack([T[a, 0] * p[:, 0] + (T[a, 1] * p[:, 1] + (T[a, 2] * p[:, 2] + T[a, 3])) for a in range(3)], axis=1)


def grid_ijk(grid, E):
    """absolute lattice indices of an oracle grid's exported leaves"""
    c = E["cell"]
    d0, d1 = int(grid.div_b[0]), int(grid.div_b[1])
    return np.stack([c % d0, (c // d0) % d1, c // (d0 * d1)], axis=1) + grid.min_b.astype(np.int64)


def centroids_in_range(grids, exports, pT, res):
    """Per transformed point: the number of centroids of all grids within one leaf size, by the f32 test the kernel
    and the oracle's KDTREE apply ((ex^2 + ey^2) + ez^2 < r^2 on the f32 centroid).  A centroid that close lies in the
    3 x 3 x 3 cells around the point's own cell, so 27 probes per grid find them all."""
    pT = np.asarray(pT, np.float32)
    inv = np.float32(1.0) / np.float32(res)
    r2 = np.float32(np.float64(np.float32(res)) * np.float64(np.float32(res)))
    fin = np.isfinite(pT).all(axis=1)
    q = np.where(fin[:, None], pT, np.float32(0))
    cell = np.floor(q * inv).astype(np.int64)
    count = np.zeros(len(pT), np.int64)
    for g, E in zip(grids, exports):
        if not len(E["cell"]):
            continue
        ijk = grid_ijk(g, E)
        lo = ijk.min(axis=0) - 2
        dims = ijk.max(axis=0) - lo + 3
        table = np.full(int(dims.prod()), -1, np.int64)
        rel = ijk - lo
        table[rel[:, 0] + dims[0] * (rel[:, 1] + dims[1] * rel[:, 2])] = np.arange(len(ijk))
        m32 = E["mean"].astype(np.float32)
        c = np.clip(cell - lo, 1, dims - 2)      # (a point clipped onto the rim is too far from every centroid)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    k = table[(c[:, 0] + dx) + dims[0] * ((c[:, 1] + dy) + dims[1] * (c[:, 2] + dz))]
                    m = m32[np.maximum(k, 0)]
                    ex, ey, ez = q[:, 0] - m[:, 0], q[:, 1] - m[:, 1], q[:, 2] - m[:, 2]
                    d = ex * ex
                    d = d + ey * ey
                    d = d + ez * ez
                    count += (k >= 0) & (d < r2) & fin
    return count


def oracle_sum(O, grids, src, pose, T, kw, hmode, pair_mode=None):
    more = dict(search_method=O.KDTREE, hessian_mode=hmode)
    if pair_mode is not None:
        more["pair_mode"] = pair_mode
    ds = [g.derivatives(src, pose, T=T, params=oprm(O, kw, **more)) for g in grids]
    return dict(score=sum(d["score"] for d in ds), gradient=sum(d["gradient"] for d in ds),
                hessian=sum(d["hessian"] for d in ds), n_pairs=sum(d["n_pairs"] for d in ds))


def check_eval(pkg, O, ndt, grids, src, poses, kw, amp=0.0, hmodes=(0, 1)):
    """The union's evaluation against the sum over the grids: tests/test_gpu_multigrid.py's assertions; `amp` widens
    them by the covariance cancellation loss exactly as tests/test_gpu_random.py does (0: not at all)."""
    poses = np.atleast_2d(poses)
    Ts = [O.pose_to_matrix(p) for p in poses]
    wide = 30 * amp
    for oh in hmodes:
        ndt.setParams(hessian_mode=pkg.HESSIAN_GAUSS_NEWTON if oh else pkg.HESSIAN_FULL)
        got = ndt.evalDerivatives(poses, transforms=Ts)
        singles = [ndt.evalDerivatives(p, transforms=[T])[0] for p, T in zip(poses, Ts)] if len(poses) > 1 else got
        for p, T, e, e1 in zip(poses, Ts, got, singles):
            d = oracle_sum(O, grids, src, p, T, kw, oh)
            x = oracle_sum(O, grids, src, p, T, kw, oh, pair_mode=2)
            print("n_pairs %d (oracle %d) score %.17g (oracle %.17g)" % (e["n_pairs"], d["n_pairs"], e["score"], d["score"]))
            assert e["n_pairs"] == d["n_pairs"] == e1["n_pairs"]
            assert e["score"] == pytest.approx(d["score"], rel=1e-8 + amp, abs=1e-9)
            assert e1["score"] == pytest.approx(d["score"], rel=1e-8 + amp, abs=1e-9)
            gn, hn = np.linalg.norm(x["gradient"]), np.linalg.norm(x["hessian"])
            rg, rh = np.linalg.norm(d["gradient"] - x["gradient"]), np.linalg.norm(d["hessian"] - x["hessian"])
            for ee in (e, e1):
                assert np.linalg.norm(ee["gradient"] - x["gradient"]) <= (1e-9 + wide) * gn + 1e-9
                assert np.linalg.norm(ee["hessian"] - x["hessian"]) <= (1e-9 + wide) * hn + 1e-9
                assert np.linalg.norm(ee["gradient"] - d["gradient"]) <= 1.01 * rg + (1e-9 + wide) * gn + 1e-9
                assert np.linalg.norm(ee["hessian"] - d["hessian"]) <= 1.01 * rh + (1e-9 + wide) * hn + 1e-9
            sc = ndt.scoreTransform(T)
            assert sc["n_pairs"] == d["n_pairs"]
            assert sc["score"] == pytest.approx(d["score"], rel=1e-8 + amp, abs=1e-9)
    return got


def check_point_sums(ndt, T):
    """tests/test_gpu_point_scores.py check_sums, for a union"""
    sc = ndt.scoreTransform(T)
    pp = ndt.scorePoints(T)
    assert int(pp["n_neighbors"].sum(dtype=np.int64)) == sc["n_pairs"]
    assert int((pp["n_neighbors"] > 0).sum()) == sc["n_points_with_neighbors"]
    assert pp["score"].sum() == pytest.approx(sc["score"], rel=1e-12)
    return pp


def check_points(O, ndt, grids, exports, src, T, sel, kw, counts=None):
    """scorePoints of a union, point by point, against the oracle grid by grid (the 1e-9 of
    tests/test_gpu_point_scores.py); the best voxel is the union cell of the best pair."""
    pp = check_point_sums(ndt, T)
    gi = ndt.getGridInfo()
    mb, db = gi["min_b"].astype(np.int64), gi["div_b"].astype(np.int64)
    d1, d2, _ = O.gauss_constants(kw["resolution"], ndt._p.outlier_ratio)
    pose6 = O.matrix_to_pose(T)
    pT = f32_transform(T, src)
    prm = oprm(O, kw, search_method=O.KDTREE)
    prm.num_threads = 1
    ijks = [grid_ijk(g, E) for g, E in zip(grids, exports)]
    if counts is not None:
        assert np.array_equal(pp["n_neighbors"], counts)      # every lane named, not only the selection
    for i in sel:
        refs = [g.derivatives(src[i:i + 1], pose6, T=T, compute_hessian=False, params=prm) for g in grids]
        n = sum(r["n_pairs"] for r in refs)
        score = sum(r["score"] for r in refs)
        assert n == pp["n_neighbors"][i], i
        assert abs(pp["score"][i] - score) <= 1e-9 * abs(score) + 1e-12, i
        nvs, bv = float(pp["nearest_voxel_score"][i]), int(pp["best_voxel"][i])
        assert (bv == -1) == (nvs == 0.0)
        pair = {}
        for g, E, ijk in zip(grids, exports, ijks):
            for r in g.neighbors(pT[i], O.KDTREE):
                x = pT[i].astype(np.float64) - E["mean"][r]
                q = float(x @ E["icov"][r] @ x)
                v = -d1 * np.exp(-d2 * 0.5 * q) if (q >= -1e-9 and d2 * q * 0.5 <= 50.0) else 0.0
                u = ijk[r] - mb
                cell = int(u[0] + db[0] * (u[1] + db[1] * u[2]))
                pair[cell] = max(pair.get(cell, 0.0), v)
        if bv == -1:
            assert all(v <= 1e-300 for v in pair.values()), i
            continue
        assert bv in pair, (i, bv)
        assert abs(pair[bv] - nvs) <= 1e-9 * nvs, (i, pair[bv], nvs)
        assert max(pair.values()) <= nvs * (1 + 1e-9), i
    return pp


def build_union(pkg, clouds, ids=None, kw=KW, **more):
    ndt = pkg.NormalDistributionsTransform(device_id=0, **dict(kw, **more))
    for k, c in enumerate(clouds):
        ndt.addTarget(c, (ids[k] if ids is not None else 100 + k))
    ndt.createVoxelKdtree()
    return ndt


# ---------------------------------------------------------------------------------------------- A: inputs (CPU)
def stacked_clouds(tgt, m, jitter, seed=11):
    """m disjoint subsamples of one cloud, each shifted by its own sub-voxel offset: every shared cell gets a chain of
    m DIFFERENT leaves"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(m):
        c = tgt[k::m]
        if jitter:
            c = c + rng.uniform(-jitter, jitter, 3).astype(np.float32)
        out.append(np.ascontiguousarray(c, np.float32))
    return out


@functools.lru_cache(maxsize=None)
def stacked_case(m, jitter=0.2):
    import __graft_entry__ as ge
    S, O = ge.load_package().synth, ge.load_oracle()
    src, tgt, _, guess = S.two_planes(step=0.05)          # 400 points per voxel and plane: 44 per grid at m = 9
    clouds = stacked_clouds(tgt, m, jitter)
    grids = [O.Grid(c, oprm(O, KW)) for c in clouds]
    exports = [g.export() for g in grids]
    pose = O.matrix_to_pose(guess)
    return dict(clouds=clouds, grids=grids, exports=exports, cand=np.ascontiguousarray(src[::3]), pose=pose,
                T=O.pose_to_matrix(pose))


LIMIT_M = 9
LIMIT_N = 8192
LIMIT_KINDS = ("lists", "walks", "one_first", "one_middle", "one_last", "mix")


@functools.lru_cache(maxsize=None)
def limit_case():
    """Sources placed on either side of the listing's limit, selected with centroids_in_range alone.
    lists: every point has <= 27 centroids in range, some exactly 27 (no lane overflows: every wave lists);
    walks: every point has >= 28, some exactly 28 (every lane overflows: every wave walks the chains);
    one_*: `lists` with ONE point of exactly 28 (one wave falls back because of one lane); mix: alternating."""
    c = stacked_case(LIMIT_M)
    cand = c["cand"]
    counts = centroids_in_range(c["grids"], c["exports"], f32_transform(c["T"], cand), KW["resolution"])

    def pick(edge, rest):
        a, b = np.flatnonzero(edge)[:LIMIT_N // 4], np.flatnonzero(rest)
        b = b[np.linspace(0, len(b) - 1, min(len(b), LIMIT_N - len(a))).astype(np.int64)] if len(b) else b
        return np.unique(np.concatenate([a, b]))

    lists = pick(counts == KD_CELLS, (counts > 0) & (counts < KD_CELLS))
    walks = pick(counts == KD_CELLS + 1, counts > KD_CELLS + 1)
    one = np.flatnonzero(counts == KD_CELLS + 1)[-1:]
    idx = dict(lists=lists, walks=walks)
    for name, pos in (("one_first", 0), ("one_middle", len(lists) // 2 + 7), ("one_last", len(lists) - 1)):
        v = lists.copy()
        if len(one) and len(v):
            v[pos] = one[0]
        idx[name] = v
    n = min(len(lists), len(walks))
    mix = np.empty(2 * n, np.int64)
    mix[0::2], mix[1::2] = lists[:n], walks[:n]
    idx["mix"] = mix
    return dict(c, counts=counts, idx=idx)


def test_limit_sources_sit_where_they_claim():
    import __graft_entry__ as ge
    O = ge.load_oracle()
    c = limit_case()
    counts, idx = c["counts"], c["idx"]
    # the helper is trusted only because its total is the oracle's
    total = sum(g.derivatives(c["cand"], c["pose"], T=c["T"], params=oprm(O, KW, search_method=O.KDTREE))["n_pairs"]
                for g in c["grids"])
    assert int(counts.sum()) == total
    print("histogram of centroids in range:", np.bincount(counts))
    for e in c["exports"]:                       # every grid has leaves of its own: chains of LIMIT_M distinct records
        assert len(e["cell"]) > 800 and (e["count"] > 0).all()
    means = np.concatenate([e["mean"] for e in c["exports"]])
    assert len(np.unique(means, axis=0)) == len(means)
    lists, walks = counts[idx["lists"]], counts[idx["walks"]]
    assert len(lists) >= 4096 and lists.max() == KD_CELLS and (lists == KD_CELLS).sum() >= 1
    assert len(walks) >= 4096 and walks.min() == KD_CELLS + 1 and (walks == KD_CELLS + 1).sum() >= 1
    for name, pos in (("one_first", 0), ("one_middle", len(lists) // 2 + 7), ("one_last", len(lists) - 1)):
        v = counts[idx[name]]
        assert len(v) == len(lists) and v[pos] == KD_CELLS + 1 and (v > KD_CELLS).sum() == 1
    mix = counts[idx["mix"]]
    assert len(mix) >= 8192 and (mix[0::2] <= KD_CELLS).all() and (mix[1::2] > KD_CELLS).all()


@pytest.mark.parametrize("m", [2, 6, 7, 9])
def test_stacked_cases_have_distinct_leaves_in_shared_cells(m):
    c = stacked_case(m)
    cells = [set(map(tuple, grid_ijk(g, e))) for g, e in zip(c["grids"], c["exports"])]
    shared = set.intersection(*cells)
    assert len(shared) > 600                      # chains of m leaves in most cells
    means = np.concatenate([e["mean"] for e in c["exports"]])
    assert len(np.unique(means, axis=0)) == len(means)


# ------------------------------------------------------------------------------------------------ A: GPU tests
@gpu
@pytest.mark.parametrize("m", [2, 6, 7, 9])
def test_distinct_stacked_grids(pkg, O, m):
    c = stacked_case(m)
    src = np.ascontiguousarray(c["cand"][::5])
    ndt = build_union(pkg, c["clouds"])
    ndt.setInputSource(src)
    rng = np.random.default_rng(m)
    poses = np.stack([c["pose"], c["pose"] + rng.normal(0, 0.02, 6), np.zeros(6)])
    check_eval(pkg, O, ndt, c["grids"], src, poses, KW)
    sel = rng.choice(len(src), 128, replace=False)
    for p in poses[:2]:
        T = O.pose_to_matrix(p)
        counts = centroids_in_range(c["grids"], c["exports"], f32_transform(T, src), KW["resolution"])
        check_points(O, ndt, c["grids"], c["exports"], src, T, sel, KW, counts=counts)


@gpu
@pytest.mark.parametrize("kind", LIMIT_KINDS)
def test_listing_limit(pkg, O, kind):
    c = limit_case()
    idx = c["idx"][kind]
    src = np.ascontiguousarray(c["cand"][idx])
    counts = c["counts"][idx]
    ndt = build_union(pkg, c["clouds"], source_order=pkg.SOURCE_ORDER_KEEP)
    ndt.setInputSource(src)
    got = check_eval(pkg, O, ndt, c["grids"], src, c["pose"], KW)
    assert got[0]["n_pairs"] == int(counts.sum())
    edge = np.flatnonzero((counts == KD_CELLS) | (counts == KD_CELLS + 1))
    rng = np.random.default_rng(5)
    sel = np.unique(np.concatenate([edge[:96], [0, len(src) // 2 + 7, len(src) - 1], rng.choice(len(src), 96, replace=False)]))
    check_points(O, ndt, c["grids"], c["exports"], src, c["T"], sel, KW, counts=counts)


def two_tiles(S, gap_cells, shift, seed=3):
    """two small tiles of the two-plane scene, `gap_cells` empty cells apart along x, with different y / z extents"""
    _, tgt, _, _ = S.two_planes(step=0.1)
    a = tgt[(tgt[:, 0] < -4) & (np.abs(tgt[:, 1]) < 5) & (np.abs(tgt[:, 2]) < 3)]
    b = tgt[(tgt[:, 0] > 4) & (tgt[:, 1] > -2) & (tgt[:, 1] < 8) & (tgt[:, 2] > -6) & (tgt[:, 2] < 2)]
    b = b + np.array([gap_cells, 0, 0], np.float32)
    sh = np.asarray(shift, np.float32)
    return [np.ascontiguousarray(a + sh, np.float32), np.ascontiguousarray(b + sh, np.float32)]


GEOMETRY = [
    # (name, resolution, min_points, gap, shift)
    ("gap-wider-than-both", 1.0, 6, 40.0, (0, 0, 0)),
    ("all-negative", 1.0, 6, 3.0, (-60.5, -45.25, -30.125)),
    ("straddling-zero", 1.0, 6, 0.0, (3.3, 0.2, 0.4)),
    ("res0.3-min3", 0.3, 3, 1.0, (-7.1, 2.2, 0.05)),
    ("res1.7-min10", 1.7, 10, 5.0, (11.0, -13.0, 2.0)),
]


@gpu
@pytest.mark.parametrize("name,res,min_pts,gap,shift", GEOMETRY, ids=[g[0] for g in GEOMETRY])
def test_union_geometry_edges(pkg, O, S, name, res, min_pts, gap, shift):
    kw = dict(KW, resolution=res, min_points_per_voxel=min_pts)
    tiles = two_tiles(S, gap, shift)
    grids = [O.Grid(t, oprm(O, kw)) for t in tiles]
    exports = [g.export() for g in grids]
    assert all(len(e["cell"]) >= 8 for e in exports)
    amp = max(float(cov_loss(e).max()) for e in exports)
    ndt = build_union(pkg, tiles, kw=kw)
    gi = ndt.getGridInfo()
    ijk = np.concatenate([grid_ijk(g, e) for g, e in zip(grids, exports)])     # the union's box is that of its LEAVES
    lo, hi = ijk.min(axis=0), ijk.max(axis=0)
    assert np.array_equal(gi["min_b"], lo) and np.array_equal(gi["div_b"], hi - lo + 1)
    base = np.concatenate([t[::7] for t in tiles])
    box_lo, box_hi = lo * np.float32(res), (hi + 1) * np.float32(res)
    # the tiles' own points, then the same cloud pushed one and two cells outside each face of the union's box, and far
    moved = [base]
    for a in range(3):
        for cells in (1, 2):
            for face, sign in ((box_lo[a], -1), (box_hi[a], 1)):
                q = base.copy()
                q[:, a] = face + sign * (cells - 0.5) * res + (base[:, a] - base[:, a].mean()) * 0.01
                moved.append(q)
    moved.append(base + np.float32(5000.0))
    src = np.ascontiguousarray(np.concatenate(moved), np.float32)
    ndt.setInputSource(src)
    rng = np.random.default_rng(1)
    poses = np.stack([np.zeros(6), rng.normal(0, 0.01, 6)])
    check_eval(pkg, O, ndt, grids, src, poses, kw, amp=amp)
    counts = centroids_in_range(grids, exports, f32_transform(np.eye(4), src), res)
    pp = check_point_sums(ndt, np.eye(4))
    assert np.array_equal(pp["n_neighbors"], counts) and counts[:len(base)].sum() > 0
    assert counts[-len(base):].sum() == 0


def expected_union_leaves(grids, exports, ids, gi):
    mb, db = gi["min_b"].astype(np.int64), gi["div_b"].astype(np.int64)
    order = np.argsort(np.asarray(ids, np.int64), kind="stable")            # ascending (signed) id
    cells, parts = [], {k: [] for k in ("count", "mean", "cov")}
    for k in order:
        u = grid_ijk(grids[k], exports[k]) - mb
        cells.append(u[:, 0] + db[0] * (u[:, 1] + db[1] * u[:, 2]))
        for f in parts:
            parts[f].append(exports[k][f])
    cell = np.concatenate(cells)
    o = np.argsort(cell, kind="stable")                                    # (union cell, ascending id)
    out = {f: np.concatenate(v)[o] for f, v in parts.items()}
    out["cell"] = cell[o]
    return out


def check_union_leaves(ndt, grids, exports, ids, clouds):
    gi = ndt.getGridInfo()
    want = expected_union_leaves(grids, exports, ids, gi)
    L = ndt.getLeaves()
    assert gi["n_leaves"] == len(want["cell"]) and gi["n_cells"] == int(gi["div_b"].astype(np.int64).prod())
    assert gi["n_target_points"] == sum(len(c) for c in clouds)
    assert np.array_equal(L["cell"], want["cell"]) and np.array_equal(L["count"], want["count"])
    np.testing.assert_allclose(L["mean"], want["mean"], rtol=1e-12, atol=0)          # tests/test_gpu_random.py
    scale = np.abs(want["cov"]).max(axis=(1, 2))
    assert ((np.abs(L["cov"] - want["cov"]).max(axis=(1, 2)) / scale) < cov_loss(want)).all()
    return L


@gpu
def test_union_export_order_and_identity(pkg, O, S):
    tiles = two_tiles(S, 0.0, (-2.5, 1.0, 0.0))
    tiles.append(np.ascontiguousarray(np.concatenate([tiles[0][::2], tiles[1][1::2]]) + np.float32(0.11)))  # overlaps both
    grids = [O.Grid(t, oprm(O, KW)) for t in tiles]
    exports = [g.export() for g in grids]
    ids = [5, -3, 2**31 + 17]                      # negative and beyond 32 bits
    ndt = build_union(pkg, tiles, ids=ids)
    La = check_union_leaves(ndt, grids, exports, ids, tiles)
    assert len(np.unique(La["cell"])) < len(La["cell"])
    src = np.ascontiguousarray(np.concatenate(tiles)[::5])
    ndt.setInputSource(src)
    check_eval(pkg, O, ndt, grids, src, np.zeros(6), KW)
    ndt.setParams(hessian_mode=pkg.HESSIAN_GAUSS_NEWTON)
    ea = ndt.evalDerivatives(np.zeros(6))[0]
    # the same tiles under the same ids in another insertion order: the same bits
    other = pkg.NormalDistributionsTransform(device_id=0, **KW)
    for k in (2, 0, 1):
        other.addTarget(tiles[k], ids[k])
    other.createVoxelKdtree()
    other.setInputSource(src)
    other.setParams(hessian_mode=pkg.HESSIAN_GAUSS_NEWTON)
    eb = other.evalDerivatives(np.zeros(6))[0]
    Lb = other.getLeaves()
    for f in ("cell", "count", "mean", "cov", "icov"):
        assert np.array_equal(La[f], Lb[f]), f
    assert eb["score"] == ea["score"] and np.array_equal(eb["gradient"], ea["gradient"]) and np.array_equal(eb["hessian"], ea["hessian"])
    # permuted ids: another chain order, the same sums within the f64 tolerance
    perm = [ids[1], ids[2], ids[0]]
    third = build_union(pkg, tiles, ids=perm)
    check_union_leaves(third, grids, exports, perm, tiles)
    third.setInputSource(src)
    check_eval(pkg, O, third, grids, src, np.zeros(6), KW)
    # replacing the cloud of an existing id is seen after the next createVoxelKdtree()
    third.addTarget(tiles[0], perm[2])             # id 5 held tiles[2]
    assert third.targetCount() == 3
    with pytest.raises(pkg.NdtError):
        third.evalDerivatives(np.zeros(6))
    third.createVoxelKdtree()
    g3, e3, t3 = [grids[0], grids[1], grids[0]], [exports[0], exports[1], exports[0]], [tiles[0], tiles[1], tiles[0]]
    check_union_leaves(third, g3, e3, perm, t3)
    check_eval(pkg, O, third, g3, src, np.zeros(6), KW)


@gpu
def test_union_rebuild_sequence_on_one_handle(pkg, O, S):
    tiles = two_tiles(S, 2.0, (0.4, -0.3, 0.2))
    grids = [O.Grid(t, oprm(O, KW)) for t in tiles]
    src = np.ascontiguousarray(np.concatenate(tiles)[::5])
    ndt = build_union(pkg, tiles)
    ndt.setInputSource(src)
    check_eval(pkg, O, ndt, grids, src, np.zeros(6), KW)
    # a plain target with a smaller box, in two neighbourhoods
    ndt.setInputTarget(tiles[1])
    for method, om in ((pkg.DIRECT7, O.DIRECT7), (pkg.KDTREE, O.KDTREE)):
        ndt.setParams(search_method=method, hessian_mode=pkg.HESSIAN_FULL)
        e = ndt.evalDerivatives(np.zeros(6))[0]
        d = grids[1].derivatives(src, np.zeros(6), params=oprm(O, KW, search_method=om))
        x = grids[1].derivatives(src, np.zeros(6), params=oprm(O, KW, search_method=om, pair_mode=2))
        assert e["n_pairs"] == d["n_pairs"] and e["score"] == pytest.approx(d["score"], rel=1e-8, abs=1e-9)
        assert np.linalg.norm(e["hessian"] - x["hessian"]) <= 1e-9 * np.linalg.norm(x["hessian"]) + 1e-9
    ndt.createVoxelKdtree()                        # the stored grids stayed
    check_eval(pkg, O, ndt, grids, src, np.zeros(6), KW)
    ndt.removeTarget(100)
    ndt.createVoxelKdtree()
    check_eval(pkg, O, ndt, grids[1:], src, np.zeros(6), KW)
    # one grid: the plain KDTREE target, bit for bit; align and alignMany agree result for result
    ref = pkg.NormalDistributionsTransform(device_id=0, search_method=pkg.KDTREE, **KW)
    ref.setInputTarget(tiles[1]); ref.setInputSource(src)
    ndt.setParams(hessian_mode=pkg.HESSIAN_FULL)
    e1, e0 = ndt.evalDerivatives(np.zeros(6))[0], ref.evalDerivatives(np.zeros(6))[0]
    assert e1["score"] == e0["score"] and np.array_equal(e1["hessian"], e0["hessian"])
    ndt.addTarget(tiles[0], 100)
    ndt.createVoxelKdtree()
    guesses = [S.pose_matrix(0.05, -0.03, 0.02, 0.0, 0.01, -0.02), np.eye(4)]
    many = ndt.alignMany(guesses)
    for g, (T, r) in zip(guesses, many):
        T1 = ndt.align(g)
        r1 = ndt.getResult()
        assert np.array_equal(T, T1) and r["score"] == r1["score"] and r["iterations"] == r1["iterations"]
    # another resolution between add and create: refused until EVERY tile has been added again
    ndt.setResolution(2.0)
    with pytest.raises(pkg.NdtError):
        ndt.createVoxelKdtree()
    ndt.addTarget(tiles[0], 100)
    with pytest.raises(pkg.NdtError):
        ndt.createVoxelKdtree()
    ndt.addTarget(tiles[1], 101)
    ndt.createVoxelKdtree()
    kw2 = dict(KW, resolution=2.0)
    check_eval(pkg, O, ndt, [O.Grid(t, oprm(O, kw2)) for t in tiles], src, np.zeros(6), kw2)


# --------------------------------------------------------------------------------------- B: keyframe archive
SCAN_SIZES = (1, 255, 256, 257, 1000, 32769)


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    R = np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def shift(x, y, z):
    T = np.eye(4)
    T[:3, 3] = [x, y, z]
    return T


BASE_POSES = {
    "identity": np.eye(4),
    "rot-x": rot(0, 2.0), "rot-y": rot(1, -2.5), "rot-z": rot(2, 3.0),
    "plus-1.5km": shift(1500.123456, -1499.987654, 3.3) @ rot(2, 0.7),
    "minus-1.5km": shift(-1500.6543, 1500.3217, -2.1) @ rot(0, 0.3) @ rot(1, -1.1),
    "40km": shift(40000.4321, 12345.6789, 51.7) @ rot(2, -2.2) @ rot(1, 0.05),
}


def f32_transform_rows(T, pts):
    """what a kernel computing in float would give: the restatement of host_transform_f64 with every operand in f32"""
    T = np.asarray(T, np.float32)
    out = np.empty_like(pts)
    for r in range(3):
        out[:, r] = ((T[r, 0] * pts[:, 0] + T[r, 1] * pts[:, 1]) + T[r, 2] * pts[:, 2]) + T[r, 3]
    return out


@functools.lru_cache(maxsize=None)
def scene():
    import __graft_entry__ as ge
    src, _, _, _ = ge.load_package().synth.two_planes(step=0.1)
    return src


def make_scan(n, seed):
    """n points of the two-plane scene; a small scan comes from one 4 m patch, so that its points share voxels with
    the other scans of a window and every one of them counts in a leaf"""
    rng = np.random.default_rng(seed)
    s = scene()
    if n < 20000:
        s = s[(np.abs(s[:, 0]) < 2) & (np.abs(s[:, 1]) < 2) & (np.abs(s[:, 2]) < 0.5)]
    p = s[rng.integers(0, len(s), n)] + rng.normal(0, 0.01, (n, 3))
    return np.ascontiguousarray(p, np.float32)


def window_poses(base, k, seed):
    rng = np.random.default_rng(seed)
    return [base @ shift(*rng.normal(0, 0.1, 3)) @ rot(2, rng.normal(0, 0.01)) for _ in range(k)]


def test_an_f32_transform_would_be_told_apart():
    scan = make_scan(32769, 1)
    for name, base in BASE_POSES.items():
        if name == "identity":
            continue
        for T in window_poses(base, 2, 4):
            a, b = host_transform_f64(T, scan), f32_transform_rows(T, scan)
            share = float((a.view(np.uint32) != b.view(np.uint32)).mean())
            print("%s: %.1f %% of the coordinates differ" % (name, 100 * share))
            assert share >= 0.01, name


def leaves_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("cell", "count", "mean", "cov", "icov"))


def check_window(pkg, O, ndt, ref, scans, ids, poses, kw, oracle=True):
    ndt.setInputTargetFromKeyframes(ids, poses)
    host = np.concatenate([host_transform_f64(T, scans[i]) for i, T in zip(ids, poses)])
    assert ndt.getGridInfo()["n_target_points"] == len(host)
    ref.setInputTarget(host)
    L, H = ndt.getLeaves(), ref.getLeaves()
    for k in ("cell", "count", "mean", "cov", "icov"):
        assert np.array_equal(L[k], H[k]), k
    if oracle:
        OL = O.Grid(host, oprm(O, kw)).export()
        assert np.array_equal(L["cell"], OL["cell"]) and np.array_equal(L["count"], OL["count"])
        if len(OL["cell"]):
            np.testing.assert_allclose(L["mean"], OL["mean"], rtol=1e-12, atol=0)
            scale = np.abs(OL["cov"]).max(axis=(1, 2))
            assert ((np.abs(L["cov"] - OL["cov"]).max(axis=(1, 2)) / scale) < cov_loss(OL)).all()
    return L


@gpu
@pytest.mark.parametrize("pose", list(BASE_POSES))
def test_window_assembly_sizes_and_poses(pkg, O, pose):
    kw = dict(KW, min_points_per_voxel=3)
    base = BASE_POSES[pose]
    ndt = pkg.NormalDistributionsTransform(device_id=0, **kw)
    ref = pkg.NormalDistributionsTransform(device_id=0, **kw)
    scans = {}
    for k, n in enumerate(SCAN_SIZES + (1000, 257, 1, 255, 256, 4097)):
        scans[k] = make_scan(n, 100 + k)
        if n > 100:                                          # non-finite points pass through and are dropped by the build
            scans[k][k] = [np.nan, 0.0, np.inf]
            scans[k][n // 2, 1] = -np.inf
        ndt.putKeyframe(k, scans[k])
    assert ndt.keyframeCount() == 12
    # windows of one keyframe of every size; the last point of a scan sits in a voxel that other scans fill
    for k in range(6):
        L = check_window(pkg, O, ndt, ref, scans, [k], window_poses(base, 1, k), kw)
        assert (len(L["cell"]) > 0) == (len(scans[k]) >= 255)
    # mixed sizes: odd destination offsets and partial blocks
    ids = [0, 1, 3, 2, 4, 5]
    L = check_window(pkg, O, ndt, ref, scans, ids, window_poses(base, 6, 7), kw)
    assert len(L["cell"]) > 100
    ids = [5, 0, 3]
    check_window(pkg, O, ndt, ref, scans, ids, window_poses(base, 3, 8), kw)
    # twelve keyframes; one id twice at two poses
    check_window(pkg, O, ndt, ref, scans, list(range(11, -1, -1)), window_poses(base, 12, 9), kw)
    check_window(pkg, O, ndt, ref, scans, [3, 5, 3, 0], window_poses(base, 4, 10), kw)


def run_archive_sequence(pkg, O, seed, mode):
    """A random life of the archive against a dict on the host; returns what was observed."""
    kw = dict(KW, min_points_per_voxel=3)
    rng = np.random.default_rng(seed)
    ndt = pkg.NormalDistributionsTransform(device_id=0, **kw)
    ndt.setHandoffMode(mode)
    ref = pkg.NormalDistributionsTransform(device_id=0, **kw)
    ref.setHandoffMode(pkg.HANDOFF_SYNC)
    model, obs, next_id = {}, [], [0]
    sizes = (255, 1000, 4097, 32769, 257, 8000)

    def put(i, n):
        model[i] = make_scan(n, int(rng.integers(1 << 30)))
        buf = model[i].copy()
        ndt.putKeyframe(i, buf)
        buf[:] = np.nan                                  # consumed when the call returns
        assert ndt.keyframeCount() == len(model)

    def fresh(n):
        next_id[0] += 1
        put(next_id[0] * 7 - 20, n)

    def erase(i):
        ndt.eraseKeyframe(i)
        del model[i]
        assert ndt.keyframeCount() == len(model)

    def big():
        return max(sorted(model), key=lambda i: len(model[i]))

    def others():
        return [i for i in sorted(model) if i != big()]

    def assemble():                                          # (the largest scan is in every window: a target with leaves)
        k = min(len(model) - 1, int(rng.integers(0, 5)))
        ids = [int(i) for i in rng.choice(others(), size=k, replace=False)] + [big()]
        ids = [ids[j] for j in rng.permutation(len(ids))]
        L = check_window(pkg, O, ndt, ref, model, ids, window_poses(np.eye(4), len(ids), int(rng.integers(1 << 30))), kw,
                         oracle=False)
        obs.append(("assemble", L["cell"].tobytes(), L["mean"].tobytes(), L["icov"].tobytes()))

    def view(then):
        i = int(rng.choice(sorted(model)))
        guess = shift(*rng.normal(0, 0.05, 3))
        ndt.setInputSourceFromKeyframe(i)
        T = ndt.align(guess)
        pp = ndt.scorePoints(T)
        scan = model[i]
        if i == big() and then in ("erase", "smaller"):
            then = "larger"
        if then == "erase":
            erase(i)
        elif then == "smaller":
            put(i, max(100, len(scan) // 3))
        elif then == "larger":
            put(i, 2 * len(scan) + 1)
        if then != "keep":
            with pytest.raises(pkg.NdtError) as ei:
                ndt.align(guess)
            assert ei.value.code == -5                       # NDT_ERR_NO_SOURCE
        ndt.setInputSource(scan)
        assert np.array_equal(ndt.align(guess), T)           # the view gave what the host scan gives
        pq = ndt.scorePoints(T)
        assert all(np.array_equal(pp[f], pq[f]) for f in pp)
        obs.append(("view", then, T.tobytes(), pp["score"].tobytes(), pp["best_voxel"].tobytes()))

    for n in sizes:
        fresh(n)
    assemble()
    view("keep")
    # six erases in a row: four pooled, the fifth and sixth released; then re-puts of every size relation to the pool
    pooled = sorted(model)
    for i in pooled:
        erase(i)
    assert ndt.keyframeCount() == 0
    for n in (255, 32769, 257, 40000, 4097, 1000, 70000):    # smaller than, equal to and larger than what is pooled
        fresh(n)
    assemble()
    view("keep")
    for _ in range(30):
        op = rng.choice(["put", "smaller", "larger", "erase", "assemble", "assemble", "view"])
        if op == "put" or len(model) < 3:
            fresh(int(rng.choice(sizes)))
        elif op in ("smaller", "larger"):
            i = int(rng.choice(others()))
            put(i, max(100, len(model[i]) // 2) if op == "smaller" else len(model[i]) + int(rng.integers(1, 3000)))
        elif op == "erase":
            erase(int(rng.choice(others())))
        elif op == "assemble":
            assemble()
        else:
            assemble()
            view(str(rng.choice(["keep", "erase", "smaller", "larger"])))
    assemble()
    return obs


@gpu
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_archive_sequences_against_a_host_model(pkg, O, seed):
    a = run_archive_sequence(pkg, O, seed, pkg.HANDOFF_SYNC)
    b = run_archive_sequence(pkg, O, seed, pkg.HANDOFF_ASYNC)
    assert len(a) == len(b) and a == b


@gpu
@pytest.mark.parametrize("mode", ["sync", "async"])
def test_empty_keyframes(pkg, O, mode):
    """include/ndt_hip.h: an empty keyframe adds nothing to a window; a window without any point is
    NDT_ERR_NO_TARGET and leaves the handle without a target (never the previous one); viewing an empty keyframe
    leaves the handle without a source."""
    kw = dict(KW, min_points_per_voxel=3)
    ndt = pkg.NormalDistributionsTransform(device_id=0, **kw)
    ndt.setHandoffMode(pkg.HANDOFF_SYNC if mode == "sync" else pkg.HANDOFF_ASYNC)
    ref = pkg.NormalDistributionsTransform(device_id=0, **kw)
    scans = {1: make_scan(1000, 1), 2: np.zeros((0, 3), np.float32), 3: make_scan(257, 3), 4: np.zeros((0, 3), np.float32)}
    for i, s in scans.items():
        ndt.putKeyframe(i, s)
    assert ndt.keyframeCount() == 4
    L = check_window(pkg, O, ndt, ref, scans, [2, 1, 4, 3, 2], window_poses(np.eye(4), 5, 1), kw)
    assert len(L["cell"]) > 0
    for ids in ([2], [2, 4, 2]):
        with pytest.raises(pkg.NdtError) as ei:
            ndt.setInputTargetFromKeyframes(ids, [np.eye(4)] * len(ids))
        assert ei.value.code == -4                           # NDT_ERR_NO_TARGET
        ndt.setInputSource(scans[1])
        with pytest.raises(pkg.NdtError) as ei:              # ... and no stale target
            ndt.align(np.eye(4))
        assert ei.value.code == -4
        check_window(pkg, O, ndt, ref, scans, [1, 2], window_poses(np.eye(4), 2, 2), kw)
    ndt.setInputSourceFromKeyframe(2)                        # an empty scan is no source
    with pytest.raises(pkg.NdtError) as ei:
        ndt.align(np.eye(4))
    assert ei.value.code == -5                               # NDT_ERR_NO_SOURCE
    ndt.eraseKeyframe(2)
    ndt.putKeyframe(2, scans[3])                             # the id is free again
    check_window(pkg, O, ndt, ref, {**scans, 2: scans[3]}, [2, 4, 1], window_poses(np.eye(4), 3, 3), kw)


# --------------------------------------------------------------------------------------------- C: downsample
def sort_passes(ncells):
    """derive_geometry (ndt_target.hip): bits = width of the cell count (the sentinel key is `ncells`), one radix pass
    per 8 bits"""
    bits = 1
    while bits < 32 and (1 << bits) <= ncells:
        bits += 1
    return (bits + 7) // 8


def pcl_cells(pts, leaf):
    p = np.asarray(pts, np.float32)
    q = p[np.isfinite(p).all(axis=1)]
    inv = np.float32(1.0) / np.float32(leaf)
    d = np.floor(q.max(0) * inv).astype(np.int64) - np.floor(q.min(0) * inv).astype(np.int64) + 1
    return int(d[0]) * int(d[1]) * int(d[2])


def crowded(n, seed=7):
    """n points inside ONE 1 m voxel far enough from the origin that every f32 addition rounds"""
    rng = np.random.default_rng(seed)
    return (np.array([100.0, -50.0, 7.0]) + rng.uniform(0.05, 0.95, (n, 3))).astype(np.float32)


def corners(extent, n_fill=6000, seed=9):
    """two corner points that span `extent` cells of 1 m per axis, plus filler inside"""
    rng = np.random.default_rng(seed)
    e = np.asarray(extent, np.float64)
    fill = rng.uniform(0, 1, (n_fill, 3)) * e
    fill[::3] = np.floor(fill[::3]) + 0.5           # (some voxels get several points)
    fill[1::3] = fill[::3][:len(fill[1::3])] + rng.uniform(-0.4, 0.4, (len(fill[1::3]), 3))
    pts = np.concatenate([[[0.25, 0.25, 0.25]], np.clip(fill, 0.01, e - 0.01), [e - 0.25]])
    return pts.astype(np.float32)


GRID_CASES = {   # name: (extent in cells, radix passes)
    "1-cell": ((1, 1, 1), 1), "2-cells": ((2, 1, 1), 1), "2^8": ((8, 8, 4), 2), "2^16": ((64, 32, 32), 3),
    "2^24": ((256, 256, 256), 4), "under-2^31": ((2047, 1024, 1023), 4),
}


def test_downsample_inputs_reach_every_pass_count():
    seen = set()
    for name, (extent, passes) in GRID_CASES.items():
        pts = corners(extent)
        n = pcl_cells(pts, 1.0)
        assert n == int(np.prod(np.asarray(extent, np.int64))) and n <= 2**31 - 1 and max(extent) < 2**24, name
        assert sort_passes(n) == passes, name
        seen.add(passes)
    assert seen == {1, 2, 3, 4}
    assert [sort_passes(c) for c in (1, 255, 256, 65535, 65536, 2**24 - 1, 2**24, 2**31 - 1)] == [1, 1, 2, 2, 3, 3, 4, 4]


def test_a_double_sum_would_be_told_apart():
    pts = crowded(200000)
    assert pcl_cells(pts, 1.0) == 1
    seq = np.cumsum(pts, axis=0, dtype=np.float32)[-1] / np.float32(len(pts))      # sequential f32, as the kernel adds
    f64 = (pts.astype(np.float64).sum(axis=0) / len(pts)).astype(np.float32)
    pair = np.array([np.ascontiguousarray(pts[:, a]).sum(dtype=np.float32) for a in range(3)]) / np.float32(len(pts))  # pairwise
    print("sequential f32", seq, "f64", f64, "pairwise f32", pair)
    assert (seq != f64).any() and (seq != pair).any()
    ref, _, counts = voxelgrid_numpy(pts[:8193], 1.0)                               # the restatement adds the same way
    assert list(counts) == [8193]
    assert np.array_equal(ref[0], np.cumsum(pts[:8193], axis=0, dtype=np.float32)[-1] / np.float32(8193))


def one_voxel_reference(pts):
    """voxelgrid_numpy for a cloud inside one voxel (its Python loop over a voxel's points, as one cumsum)"""
    return (np.cumsum(pts, axis=0, dtype=np.float32)[-1] / np.float32(len(pts)))[None, :]


def download(hipmem, ptr, n, dtype=np.float32):
    a = np.zeros(n, dtype)
    if n:
        assert hipmem.rt.hipMemcpy(a.ctypes.data, C.c_void_p(ptr), a.nbytes, 2) == 0
    return a


def device_downsample(ndt, hipmem, pts, leaf, inten=None, cap=None, sentinel=-777.0):
    n = len(pts)
    d = [hipmem.upload(np.ascontiguousarray(pts[:, a])) for a in range(3)]
    di = hipmem.upload(inten) if inten is not None else None
    o = [hipmem.upload(np.full(n, sentinel, np.float32)) for _ in range(4)]
    m = ndt.voxelDownsampleDevice(d[0], d[1], d[2], n, leaf, o[0], o[1], o[2], n if cap is None else cap,
                                  d_intensity=di, o_intensity=o[3] if inten is not None else None)
    return m, o, d


@gpu
@pytest.mark.parametrize("n", [1, 2, 257, 8193, 200000])
def test_downsample_one_crowded_voxel(pkg, hipmem, n):
    pts = crowded(200000)[:n]
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    ref = one_voxel_reference(pts)
    if n <= 8193:
        full, _, counts = voxelgrid_numpy(pts, 1.0)
        assert np.array_equal(full, ref) and list(counts) == [n]
    assert np.array_equal(ndt.voxelDownsample(pts, 1.0), ref)
    inten = np.random.default_rng(n).uniform(0, 255, n).astype(np.float32)
    m, o, _ = device_downsample(ndt, hipmem, pts, 1.0, inten=inten)
    assert m == 1
    got = np.array([download(hipmem, o[a], 1)[0] for a in range(4)])
    assert np.array_equal(got[:3], ref[0])
    assert got[3] == np.cumsum(inten, dtype=np.float32)[-1] / np.float32(n)


@gpu
def test_downsample_one_voxel_holds_half_the_cloud(pkg, hipmem):
    rng = np.random.default_rng(3)
    heavy = crowded(50000)
    rest = (np.array([100.0, -50.0, 7.0]) + rng.uniform(-10, 10, (50000, 3))).astype(np.float32)
    pts = np.concatenate([heavy, rest])[rng.permutation(100000)]
    ref, _, counts = voxelgrid_numpy(pts, 1.0)
    assert counts.max() >= 50000 and len(counts) > 5000
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    assert np.array_equal(ndt.voxelDownsample(pts, 1.0), ref)


@gpu
@pytest.mark.parametrize("name", list(GRID_CASES))
def test_downsample_every_radix_pass_count(pkg, hipmem, name):
    pts = corners(GRID_CASES[name][0])
    ref, _, _ = voxelgrid_numpy(pts, 1.0)
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    assert np.array_equal(ndt.voxelDownsample(pts, 1.0), ref)
    m, o, _ = device_downsample(ndt, hipmem, pts, 1.0)
    assert m == len(ref)
    assert np.array_equal(np.stack([download(hipmem, o[a], m) for a in range(3)], axis=1), ref)


@gpu
@pytest.mark.parametrize("n,leaf", [(8191, 0.3), (8192, 1.7), (8193, 0.3), (65536, 1.7), (100003, 0.3)])
def test_downsample_sizes_negative_coordinates_and_capacity(pkg, hipmem, n, leaf):
    rng = np.random.default_rng(n)
    pts = rng.uniform(-9.0, 3.0, (n, 3)).astype(np.float32)
    pts[:, 2] *= np.float32(0.2)
    pts[::97] = np.nan
    inten = rng.uniform(0, 255, n).astype(np.float32)
    ref, ref_i, _ = voxelgrid_numpy(pts, leaf, inten)
    n_out = len(ref)
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    assert np.array_equal(ndt.voxelDownsample(pts, leaf), ref)
    # intensity present, capacity exactly n_out: nothing beyond it is written
    m, o, d = device_downsample(ndt, hipmem, pts, leaf, inten=inten, cap=n_out)
    assert m == n_out
    for a in range(4):
        back = download(hipmem, o[a], n)
        assert np.array_equal(back[:n_out], ref[:, a] if a < 3 else ref_i)
        assert (back[n_out:] == np.float32(-777.0)).all()
    # intensity absent
    m, o2, _ = device_downsample(ndt, hipmem, pts, leaf)
    assert m == n_out and np.array_equal(np.stack([download(hipmem, o2[a], m) for a in range(3)], axis=1), ref)
    # one short: refused, the message names n_out, and the first cap entries are all that was touched
    o3 = [hipmem.upload(np.full(n, -777.0, np.float32)) for _ in range(3)]
    with pytest.raises(pkg.NdtError) as ei:
        ndt.voxelDownsampleDevice(d[0], d[1], d[2], n, leaf, o3[0], o3[1], o3[2], n_out - 1)
    assert ei.value.code == -1 and str(n_out) in str(ei.value)
    for a in range(3):
        assert (download(hipmem, o3[a], n)[n_out - 1:] == np.float32(-777.0)).all()
    # the device output as a target without a host round trip; as a grid of a union and as a keyframe (both take host
    # clouds) from its copy: the leaves of the reference cloud
    kw = dict(KW, resolution=4 * leaf, min_points_per_voxel=3)     # (voxels that hold dozens of the centroids)
    a, b = pkg.NormalDistributionsTransform(device_id=0, **kw), pkg.NormalDistributionsTransform(device_id=0, **kw)
    a.setInputTargetDevice(o2[0], o2[1], o2[2], n_out)
    b.setInputTarget(ref)
    La, Lb = a.getLeaves(), b.getLeaves()
    assert leaves_equal(La, Lb) and len(Lb["cell"]) > 0
    out = np.stack([download(hipmem, o2[k], n_out) for k in range(3)], axis=1)
    a.putKeyframe(1, out)
    a.setInputTargetFromKeyframes([1], [np.eye(4)])
    assert leaves_equal(a.getLeaves(), Lb)
    a.addTarget(out, 1)
    a.createVoxelKdtree()
    Lu = a.getLeaves()
    assert all(np.array_equal(Lu[k], Lb[k]) for k in ("count", "mean", "cov"))      # (cells are relative to the union's box)


@gpu
def test_downsample_no_capacity_on_an_all_nan_cloud(pkg, hipmem):
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    pts = np.full((1000, 3), np.nan, np.float32)
    d = [hipmem.upload(np.ascontiguousarray(pts[:, a])) for a in range(3)]
    assert ndt.voxelDownsampleDevice(d[0], d[1], d[2], len(pts), 0.5, None, None, None, 0) == 0
