"""The clouds GICP's point index is tested against at its edges (tests/test_gpu_gicp_edges.py runs them on the device), and
the proof, without a GPU, that each of them is the hard case it is meant to be: a later change to a cloud then cannot
silently remove the case.  The yardstick is tests/test_gicp_cpu.py's, unchanged (knn_brute, cov_numpy, reg_cov_numpy,
pairs_brute, gicp_numpy, gicp_align_numpy).  One restatement is added: `index_geometry`, the bounding box, cell edge and
cell counts as fit_build_cloud (ndt_fitness.hip) derives them, with `cell_coordinates` for fit_cell (ndt_fit_device.h).

  1  the integer lattice of knn_cloud translated to +-16 km / +-32 km, and scaled by 1/4: every coordinate stays exact in
     f32, so the expected lists are those of the lattice at the origin; at cell edges 0.3 and 0.7 (inv_c inexact) points
     are classified into another cell than exact arithmetic puts them in
  2  a jittered wavy sheet at 20 km and at coordinates that are not exact in f32
  3  degenerate extents: one point 100 times, a line, a plane, exactly four finite points
  4  two blobs 190 m apart at cell edges of 0.1 and 0.03: the cell edge grows, no point settles in its 27 cells
  5  the CT scene under a finite neighbour cap: points without a covariance on both sides, pairs dropped for that
  6  a source outside the target's bounding box on every side, and 1e6 m out
  7  the restatement's own rules for what is not finite"""
import functools

import numpy as np
import pytest

from test_ct_cpu import scene
from test_d2d_cpu import ATTITUDE
from test_gicp_cpu import (DEFAULTS, GAP_MIN, KS, MIN_NEIGHBOURS, cov_numpy, gicp_align_numpy, gicp_numpy, knn_brute, knn_cloud,
                           pairs_brute, reg_cov_numpy, scene_neighbours, sym3)

F32 = np.float32
POSE_GENERAL = np.array([0.16, 0.03, 0.05, 0.004, -0.003, 0.054])          # tests/test_gpu_gicp.py's
POSE_ATT = np.array([*POSE_GENERAL[:3], *ATTITUDE])
EDGES = (1.0, 0.5, 0.3, 0.7)                                                 # 0.3 and 0.7: inv_c = 1.0f / c is inexact
CELL_LIMIT = float(1 << 30)


# ---- the index's geometry -----------------------------------------------------------------------------------------------
def index_geometry(cloud, resolution):
    """(lo [3] f32, c f32, inv_c f32, dims [3] int, growth_steps) as fit_build_cloud computes them: the bounding box of the
    finite points, dims = floor((hi - lo) * inv_c) + 1 in f32, and c *= 1.25f while the box has 2^30 cells or more"""
    p = np.ascontiguousarray(cloud, F32)
    p = p[np.isfinite(p).all(axis=1)]
    lo, hi = p.min(axis=0), p.max(axis=0)
    c, steps = F32(resolution), 0
    while True:
        inv_c = F32(1.0) / c
        u = (hi - lo) * inv_c                                                # float32
        d = np.floor(u).astype(np.float64) + 1.0
        if d.prod() < CELL_LIMIT:
            return lo, c, inv_c, d.astype(np.int64), steps
        c = c * F32(1.25)
        steps += 1


def cell_coordinates(points, lo, inv_c, dims):
    """(k32, k64) [n, 3]: fit_cell's floor((p - lo) * inv_c) clamped to [-1, dims] in f32 as the device evaluates it, and the
    same expression of the same f32 inputs in f64"""
    p = np.ascontiguousarray(points, F32)
    with np.errstate(all="ignore"):
        k32 = np.clip(np.floor((p - lo) * inv_c), F32(-1.0), dims.astype(F32))
        k64 = np.clip(np.floor((p.astype(np.float64) - lo.astype(np.float64)) * np.float64(inv_c)), -1.0, dims.astype(np.float64))
    return k32.astype(np.int64), k64.astype(np.int64)


# ---- 1. translated lattices ---------------------------------------------------------------------------------------------
OFFSETS = {"A": (16384.0, -8192.0, 2048.0), "B": (-32768.0, 32768.0, -4096.0)}
LATTICE_SCALE = 0.25
LATTICE_SIZES = (257, 4099)
CAP_DIAGONAL = np.sqrt(2.0) * LATTICE_SCALE                                  # (float)(cap * cap) == 0.125: the face diagonal's d2


def lattice_edges(scaled):
    """the cell edges a lattice cloud is indexed at: EDGES and the one that stands in where 0.7 cannot mis-classify
    (test_inexact_edges_misclassify_lattice_points)"""
    return EDGES + ((0.15,) if scaled else (0.6,))


def lattice(n, offset, scaled=False):
    """knn_cloud(n), scaled by 1/4 or not, moved by OFFSETS[offset]; float64, exactly representable in f32"""
    p = knn_cloud(n).astype(np.float64)
    return (p * LATTICE_SCALE if scaled else p) + np.array(OFFSETS[offset])


# ---- 2. a generic surface at km scale -----------------------------------------------------------------------------------
SHEET_N = 4099
SHEET_OFFSETS = {"origin": (0.0, 0.0, 0.0), "km20": (20000.0, -20000.0, 300.0), "inexact": (-8191.7, 4095.9, -12.3)}


def sheet(offset):
    """4099 points of a jittered wavy sheet, x, y uniform in [0, 12), z = 0.3 sin x + 0.02 N(0, 1), moved and cast to f32"""
    rng = np.random.default_rng(41)
    x, y = rng.uniform(0.0, 12.0, SHEET_N), rng.uniform(0.0, 12.0, SHEET_N)
    z = 0.3 * np.sin(x) + 0.02 * rng.normal(0.0, 1.0, SHEET_N)
    return (np.stack([x, y, z], axis=1) + np.array(SHEET_OFFSETS[offset])).astype(F32)


# ---- 3. degenerate extents ----------------------------------------------------------------------------------------------
def degenerate(which):
    if which == "point":                                                     # 100 copies of one point: dims 1 x 1 x 1
        return np.tile(np.array([3.7, -1.3, 0.9], F32), (100, 1))
    if which == "line":                                                      # 300 collinear points: dims N x 1 x 1
        return np.stack([0.125 * np.arange(300), np.full(300, 2.5), np.full(300, -1.25)], axis=1).astype(F32)
    if which == "plane":                                                     # a 40 x 40 grid: dims N x M x 1
        i, j = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
        return np.stack([0.125 * i.ravel(), 0.125 * j.ravel() - 2.0, np.full(1600, 0.75)], axis=1).astype(F32)
    four = np.array([[0.5, 0.25, 0.0], [1.75, -0.5, 0.125], [0.0, 2.0, 1.5], [-1.25, 0.75, 2.5]], F32)
    if which == "four":                                                      # the smallest cloud that has a covariance
        return four
    if which == "five":                                                      # ... and with a point that is not finite
        return np.concatenate([four[:2], np.array([[0.0, np.nan, 0.0]], F32), four[2:]])
    raise KeyError(which)


DEGENERATE = ("point", "line", "plane", "four", "five")


# ---- 4. the growth clouds -----------------------------------------------------------------------------------------------
GROWTH_EDGES = (0.1, 0.03)
GROWTH_KS = (20, 32)
BLOB = 300


def growth_cloud(strays=False):
    """two blobs of 300 points, uniform in a cube of 0.6 m, at (0, 0, 0) and (110, 110, 110); with `strays` three points
    near (55, 55, 55) more than 1 m apart (only ever searched under a neighbour cap of 1 m)"""
    rng = np.random.default_rng(2)
    a = rng.uniform(0.0, 0.6, (BLOB, 3))
    b = rng.uniform(0.0, 0.6, (BLOB, 3)) + 110.0
    parts = [a, b]
    if strays:
        parts.append(np.array([[55.0, 55.0, 55.0], [56.5, 55.25, 54.0], [53.75, 56.5, 55.5]]))
    return np.concatenate(parts).astype(F32)


# ---- 5 / 6. the scene, its neighbour caps and a source outside its box ---------------------------------------------------
CAPS = (0.5, 0.8)
D_SCENE = 5.0
SCENE_SHIFT = np.array([3000.0, -3000.0, 40.0])
# what the yardstick gives on the scene at POSE_GENERAL, k = 20, D = 5: target points without a covariance, source points
# without, pairs, and pairs dropped only because the nearest target point has no covariance
CAP_TABLE = {0.5: dict(target_without=1023, source_without=1475, pairs=2609, dropped_for_target=416),
             0.8: dict(target_without=23, source_without=167, pairs=4323, dropped_for_target=10)}
OUTSIDE_K, OUTSIDE_CAP = 4, 200.0                                            # the source-side rule `outside_source` is run under
FAR_OUT = 1.0e6


def scene_target(shifted=False):
    t = scene()["target"]
    return (t.astype(np.float64) + SCENE_SHIFT).astype(F32) if shifted else t


def scene_source(turned=False):
    """the rigid scan; `turned`: turned back by ATTITUDE's inverse, so that POSE_ATT puts it on the target"""
    from slam_sam_amd import synth
    s = scene()["ideal"]
    return synth.transform(np.linalg.inv(synth.pose_matrix(0, 0, 0, *ATTITUDE)), s).astype(F32) if turned else s


def shifted_pose(pose6):
    return np.concatenate([np.asarray(pose6[:3]) + SCENE_SHIFT, pose6[3:]])


def outside_source(shifted=False):
    """32 points: 40 m out from the centre of the target's box along each axis (0..5) and at the 8 corners (6..13), two
    clusters of four points 1e6 m out on +x (14..17) and on -z (18..21), and ten ordinary scan points (22..31).
    The far points come in fours so that each has a covariance under k_neighbours = 4: a lone point that far out would
    make its own neighbour search walk the source index's whole box, about 2^30 cells."""
    t = scene_target(shifted).astype(np.float64)
    centre = 0.5 * (t.min(axis=0) + t.max(axis=0))
    axes = np.concatenate([np.eye(3), -np.eye(3)]) * 40.0
    corners = np.array([[sx, sy, sz] for sx in (-40.0, 40.0) for sy in (-40.0, 40.0) for sz in (-40.0, 40.0)])
    four = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.25, 0.0], [0.0, 0.0, 0.25]])
    far_x = np.array([FAR_OUT, 0.0, 0.0]) + four
    far_z = np.array([0.0, 0.0, -FAR_OUT]) + four
    special = np.concatenate([axes, corners, far_x, far_z]) + centre
    ordinary = scene()["ideal"][100:110].astype(np.float64) + (SCENE_SHIFT if shifted else 0.0)
    return np.concatenate([special, ordinary]).astype(F32)


# ---- brute force, computed once ------------------------------------------------------------------------------------------
CLOUDS = {}
for _n in LATTICE_SIZES:
    for _o in OFFSETS:
        for _s in (False, True):
            CLOUDS["lattice-%s%s-%d" % (_o, "-quarter" if _s else "", _n)] = functools.partial(lattice, _n, _o, _s)
for _o in SHEET_OFFSETS:
    CLOUDS["sheet-%s" % _o] = functools.partial(sheet, _o)
for _w in DEGENERATE:
    CLOUDS["degenerate-%s" % _w] = functools.partial(degenerate, _w)
CLOUDS["growth"] = growth_cloud
CLOUDS["growth-strays"] = functools.partial(growth_cloud, True)
CLOUDS["scene-target"] = scene_target
CLOUDS["scene-target-shifted"] = functools.partial(scene_target, True)
CLOUDS["scene-source"] = scene_source
CLOUDS["scene-source-turned"] = functools.partial(scene_source, True)
CLOUDS["outside"] = outside_source
CLOUDS["outside-shifted"] = functools.partial(outside_source, True)


@functools.lru_cache(maxsize=None)
def cloud_of(name):
    p = np.ascontiguousarray(CLOUDS[name](), F32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def lattice_lists(n, k, cap):
    return knn_brute(knn_cloud(n), k, cap)


@functools.lru_cache(maxsize=None)
def brute(name, k, cap=np.inf):
    """dict(idx, found, mean, raw) of CLOUDS[name] by brute force, computed once and left unchanged"""
    cloud = cloud_of(name)
    if name.startswith("lattice-"):
        # the lists of the lattice at the origin (test_translated_lattices_keep_their_lists: equal index for index)
        idx, found = lattice_lists(int(name.rsplit("-", 1)[1]), k, cap / (LATTICE_SCALE if "-quarter" in name else 1.0))
    else:
        idx, found = knn_brute(cloud, k, cap)
    mean, raw = cov_numpy(cloud, idx, found)
    for a in (idx, found, mean, raw):
        a.setflags(write=False)
    return dict(idx=idx, found=found, mean=mean, raw=raw)


def scene_setting(setting):
    """(target name, source name, pose) of the three pairings of the scene"""
    return {"general": ("scene-target", "scene-source", POSE_GENERAL),
            "attitude": ("scene-target", "scene-source-turned", POSE_ATT),
            "shifted": ("scene-target-shifted", "scene-source", shifted_pose(POSE_GENERAL))}[setting]


@functools.lru_cache(maxsize=None)
def scene_pairs(setting, cap, D=D_SCENE):
    """dict(pair, d2, dropped_for_target, sfound, tfound): pairs_brute of the scene under the neighbour cap, and how many pairs
    it drops only because the nearest target point has no covariance"""
    tname, sname, pose = scene_setting(setting)
    sfound, tfound = brute(sname, 20, cap)["found"], brute(tname, 20, cap)["found"]
    pair, d2 = pairs_brute(pose, cloud_of(sname), sfound, cloud_of(tname), tfound, D)
    free, _ = pairs_brute(pose, cloud_of(sname), sfound, cloud_of(tname), np.full(len(tfound), 20, np.int32), D)
    assert ((pair >= 0) <= (free >= 0)).all() and np.array_equal(pair[pair >= 0], free[pair >= 0])
    return dict(pair=pair, d2=d2, dropped_for_target=int((free >= 0).sum() - (pair >= 0).sum()), sfound=sfound, tfound=tfound)


# ---- the checks -----------------------------------------------------------------------------------------------------------
def test_index_geometry_restates_the_build():
    """an exact edge, no growth: the lattice of side 17 with the far point at 500 m; and the bound of 2^30 cells itself"""
    lo, c, inv_c, dims, steps = index_geometry(knn_cloud(4099), 0.5)
    assert steps == 0 and c == F32(0.5) and inv_c == F32(2.0) and dims.tolist() == [1001, 33, 33] and (lo == 0).all()
    two = np.array([[0.0, 0.0, 0.0], [1023.0, 1023.0, 1023.0]], F32)          # 1024^3 = 2^30 cells: one step
    assert index_geometry(two, 1.0)[4] == 1 and index_geometry(two, 1.0)[1] == F32(1.25)
    assert index_geometry(two[:, :] * F32(1022.0 / 1023.0), 1.0)[4] == 0      # 1023^3: none


@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "quarter"])
@pytest.mark.parametrize("offset", list(OFFSETS))
@pytest.mark.parametrize("n", LATTICE_SIZES)
def test_translated_lattices_keep_their_lists(n, offset, scaled):
    """the cast to f32 loses nothing and every difference of two coordinates is exact, so brute force gives the lists of the
    lattice at the origin index for index: the expected lists are known twice"""
    p64 = lattice(n, offset, scaled)
    p = p64.astype(F32)
    fin = np.isfinite(p64).all(axis=1)
    assert np.array_equal(p.astype(np.float64)[fin], p64[fin]) and np.array_equal(np.isnan(p), np.isnan(p64))
    name = "lattice-%s%s-%d" % (offset, "-quarter" if scaled else "", n)
    assert np.array_equal(cloud_of(name)[fin], p[fin])
    scale = LATTICE_SCALE if scaled else 1.0
    for k in KS:
        for cap in (np.inf, 1.0) + ((CAP_DIAGONAL,) if scaled else ()):
            base = lattice_lists(n, k, cap / scale)
            got = knn_brute(p, k, cap)                                        # brute force over the translated cloud itself
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), (k, cap)
            assert brute(name, k, cap)["idx"] is not None
    if scaled:
        # the inclusive rule decides: (float)(cap * cap) is exactly the d2 of the face diagonal, 0.125
        assert F32(CAP_DIAGONAL * CAP_DIAGONAL) == F32(0.125)
        idx, found = brute(name, 32, CAP_DIAGONAL)["idx"], brute(name, 32, CAP_DIAGONAL)["found"]
        x = p.astype(np.float64)
        d2 = ((x[np.where(idx >= 0, idx, 0)] - x[:, None, :]) ** 2).sum(axis=2)
        on_cap = (d2 == 0.125) & (idx >= 0)
        assert on_cap.sum() > n                                               # diagonal neighbours exactly on the cap: kept
        assert (found[fin] < 32).all() and found[fin].max() >= 19 - 1         # 1 + 6 + 12 lattice neighbours at the most, and duplicates
        below = knn_brute(p, 32, float(np.nextafter(F32(CAP_DIAGONAL), F32(0))) * (1.0 - 1e-7))[1]
        assert (below[fin] < found[fin]).any()                                # a cap one step shorter drops them


@pytest.mark.parametrize("edge", (0.3, 0.7, 0.6, 0.15))
def test_inexact_edges_misclassify_lattice_points(edge):
    """At cell edges whose reciprocal is inexact in f32, points of the translated lattices land in another cell than the
    same expression gives in f64: the mis-classification the slack of fit_lower_bound2 is there for.  It happens at 0.3 on
    every lattice cloud.  It cannot happen at 0.7 under ANY translation that keeps the coordinates exact: p - lo is then
    the lattice's own difference whatever the offset, (float)(1 / 0.7f) lies ABOVE 10 / 7, so a product that is an integer
    in exact arithmetic (p - lo a multiple of 7) lies just above it and rounds down onto it: the same cell.  A third offset
    cannot change that, so a third EDGE stands in for it: 0.6 for the unit lattices and 0.15 for the quarter lattices (their
    f32 reciprocals lie BELOW 5 / 3 and 20 / 3, and the product rounds up onto the integer); the device tests run those
    edges beside 0.3 and 0.7."""
    inv = F32(1.0) / F32(edge)
    assert np.float64(inv) * np.float64(F32(edge)) != 1.0
    for n in LATTICE_SIZES:
        for offset in OFFSETS:
            for scaled in (False, True):
                if edge != lattice_edges(scaled)[-1] and edge in (0.6, 0.15):
                    continue
                p = cloud_of("lattice-%s%s-%d" % (offset, "-quarter" if scaled else "", n))
                lo, c, inv_c, dims, steps = index_geometry(p, edge)
                assert steps == 0 and c == F32(edge)
                fin = np.isfinite(p).all(axis=1)
                k32, k64 = cell_coordinates(p[fin], lo, inv_c, dims)
                wrong = (k32 != k64).any(axis=1)
                print("edge %.2f, lattice %s%s %d: %d of %d points in another cell than f64 puts them" %
                      (edge, offset, " / 4" if scaled else "", n, wrong.sum(), fin.sum()))
                assert (wrong.sum() == 0) if edge == 0.7 else (wrong.sum() >= n // 4)
                assert (k32 >= 0).all() and (k32 < dims).all()                # the cloud's own points: inside its box


@pytest.mark.parametrize("offset", list(SHEET_OFFSETS))
def test_sheet_is_generic(offset):
    """all points distinct after the cast, 20 neighbours each, and none of them below the gap the regularised covariance is
    compared above"""
    name = "sheet-%s" % offset
    p = cloud_of(name)
    assert p.shape == (SHEET_N, 3) and np.isfinite(p).all()
    assert len(np.unique(p, axis=0)) == SHEET_N
    if offset != "origin":
        assert np.abs(p).max() > 8000.0
    b = brute(name, 20)
    assert (b["found"] == 20).all()
    _, gap = reg_cov_numpy(b["raw"], DEFAULTS["covariance_epsilon"])
    print("%s: %.4f of the points below the gap, smallest gap %.3e" % (name, (gap < GAP_MIN).mean(), gap.min()))
    assert (gap >= GAP_MIN).all()
    for edge in EDGES:
        assert index_geometry(p, edge)[4] == 0


def test_degenerate_extents():
    eps = DEFAULTS["covariance_epsilon"]
    # (a) one point 100 times
    p = cloud_of("degenerate-point")
    assert index_geometry(p, 1.0)[3].tolist() == [1, 1, 1] and index_geometry(p, 0.3)[3].tolist() == [1, 1, 1]
    for k in KS:
        b = brute("degenerate-point", k)
        assert (b["idx"] == np.arange(k)[None, :]).all() and (b["found"] == k).all()
        assert (b["raw"] == 0.0).all() and np.array_equal(b["mean"], np.tile(p[0].astype(np.float64), (100, 1)))
    # (b) a line, (c) a plane
    p = cloud_of("degenerate-line")
    assert index_geometry(p, 1.0)[3].tolist() == [38, 1, 1] and index_geometry(p, 0.3)[3][1:].tolist() == [1, 1]
    q = cloud_of("degenerate-plane")
    assert index_geometry(q, 1.0)[3].tolist() == [5, 5, 1] and index_geometry(q, 0.3)[3][2] == 1
    for k in KS:
        for name, rank in (("degenerate-line", 1), ("degenerate-plane", 2)):
            b = brute(name, k)
            assert (b["found"] == k).all()
            assert (np.linalg.matrix_rank(sym3(b["raw"])) == rank).all(), (name, k)
    raw = brute("degenerate-plane", 20)["raw"]
    assert (raw[:, [2, 4, 5]] == 0.0).all()                                   # nothing along z, exactly
    Cm, _ = reg_cov_numpy(raw, eps)
    assert np.abs(np.abs(Cm[:, 2, 2]) - eps).max() < 1e-15                     # the normal is +-z
    # (d) exactly four finite points
    for name, n_fin in (("degenerate-four", 4), ("degenerate-five", 4)):
        c = cloud_of(name)
        fin = np.isfinite(c).all(axis=1)
        assert fin.sum() == n_fin == MIN_NEIGHBOURS
        for k in KS:
            b = brute(name, k)
            assert (b["found"][fin] == 4).all() and (b["found"][~fin] == 0).all() and np.isfinite(b["raw"][fin]).all()
            assert np.isnan(b["raw"][~fin]).all()
        assert (np.linalg.matrix_rank(sym3(brute(name, 4)["raw"][fin])) == 3).all()


@pytest.mark.parametrize("edge", GROWTH_EDGES)
def test_growth_clouds_grow_the_cell_edge(edge):
    """the cell edge grows (once at 0.1 m to 885^3 cells, six times at 0.03 m), and every point's k-th neighbour lies within 3
    final cell edges, for many points beyond 2: pass 1 queues those, and the queue settles every point in a few shells"""
    p = cloud_of("growth")
    lo, c, inv_c, dims, steps = index_geometry(p, edge)
    assert steps == {0.1: 1, 0.03: 6}[edge] and dims.prod() < CELL_LIMIT
    assert c == F32(edge) * F32(1.25) if steps == 1 else c > F32(edge) * F32(3.0)
    if edge == 0.1:
        assert dims.tolist() == [885, 885, 885]
    x = p.astype(np.float64)
    for k in GROWTH_KS:
        b = brute("growth", k)
        assert (b["found"] == k).all()
        kth = np.sqrt(((x[b["idx"][:, k - 1]] - x) ** 2).sum(axis=1)) / float(c)
        print("edge %.2f (grown to %.4f, %d steps, dims %s), k = %d: k-th neighbour between %.2f and %.2f cell edges away"
              % (edge, c, steps, dims.tolist(), k, kth.min(), kth.max()))
        assert kth.max() <= 3.0
        assert kth.min() > 1.0                                                # (never within the bound of the 27 cells)
        same_blob = (b["idx"] < BLOB) == (np.arange(2 * BLOB) < BLOB)[:, None]
        assert same_blob.all()


def test_growth_strays_have_no_covariance_under_the_cap():
    p = cloud_of("growth-strays")
    assert len(p) == 2 * BLOB + 3 and index_geometry(p, 0.1)[4] == 1
    for k in GROWTH_KS:
        found = brute("growth-strays", k, 1.0)["found"]
        assert (found[:2 * BLOB] == k).all() and (found[2 * BLOB:] < MIN_NEIGHBOURS).all()
        assert np.isnan(brute("growth-strays", k, 1.0)["raw"][2 * BLOB:]).all()


@pytest.mark.parametrize("cap", CAPS)
def test_neighbour_cap_on_the_scene(pkg, cap):
    """the counts the yardstick gives at POSE_GENERAL, k = 20, D = 5; at the cap of 0.5 m the rule "the nearest target point
    has no covariance: the pair is dropped, not replaced" decides for hundreds of pairs"""
    r = scene_pairs("general", cap)
    got = dict(target_without=int((r["tfound"] < MIN_NEIGHBOURS).sum()), source_without=int((r["sfound"] < MIN_NEIGHBOURS).sum()),
               pairs=int((r["pair"] >= 0).sum()), dropped_for_target=r["dropped_for_target"])
    print("cap %.1f: %s" % (cap, got))
    assert got == CAP_TABLE[cap]
    if cap == 0.5:
        assert got["dropped_for_target"] >= 100 and got["pairs"] >= 2000
    for setting in ("attitude", "shifted"):
        o = scene_pairs(setting, cap)
        print("cap %.1f, %s: %d pairs, %d dropped for the target point alone" % (cap, setting, (o["pair"] >= 0).sum(), o["dropped_for_target"]))
        assert (o["pair"] >= 0).sum() > 2000 and o["dropped_for_target"] >= (100 if cap == 0.5 else 1)


def test_the_shifted_scene_is_not_the_scene_moved(pkg):
    """3 km out the cast rounds the target's points: its lists are its own, not the scene's"""
    t, s = cloud_of("scene-target"), cloud_of("scene-target-shifted")
    assert not np.array_equal((s.astype(np.float64) - SCENE_SHIFT), t.astype(np.float64))
    assert np.abs(s.astype(np.float64) - SCENE_SHIFT - t).max() < 2e-4
    assert not np.array_equal(brute("scene-target-shifted", 20)["idx"], brute("scene-target", 20)["idx"])


@pytest.mark.parametrize("shifted", [False, True], ids=["scene", "shifted"])
def test_outside_source_meets_both_clamps_on_every_axis(pkg, shifted):
    tname = "scene-target-shifted" if shifted else "scene-target"
    src = cloud_of("outside-shifted" if shifted else "outside")
    assert src.shape == (32, 3) and np.isfinite(src).all()
    lo, c, inv_c, dims, steps = index_geometry(cloud_of(tname), 1.0)
    assert steps == 0
    k32, _ = cell_coordinates(src, lo, inv_c, dims)                          # the identity pose: the moved point is the point
    for a in range(3):
        assert (k32[:, a] == -1).any() and (k32[:, a] == dims[a]).any(), a
    inside = ((k32 >= 0) & (k32 < dims)).all(axis=1)
    assert inside[22:].all() and not inside[:22].any()
    assert np.abs(src[14:18, 0]).min() > 0.9 * FAR_OUT and np.abs(src[18:22, 2]).min() > 0.9 * FAR_OUT
    # every point has a covariance under the source-side rule the device test runs it with, and settles near by
    b = brute("outside-shifted" if shifted else "outside", OUTSIDE_K, OUTSIDE_CAP)
    assert (b["found"] == OUTSIDE_K).all()
    assert index_geometry(src, 1.0)[4] > 10                                   # the source's own index grows its cells
    assert set(b["idx"][14:18].ravel()) == {14, 15, 16, 17} and set(b["idx"][18:22].ravel()) == {18, 19, 20, 21}
    tfound = brute(tname, OUTSIDE_K, OUTSIDE_CAP)["found"]
    assert (tfound == OUTSIDE_K).all()
    pose = np.zeros(6)
    near, _ = pairs_brute(pose, src, b["found"], cloud_of(tname), tfound, D_SCENE)
    every, d2 = pairs_brute(pose, src, b["found"], cloud_of(tname), tfound, np.inf)
    assert (near[:22] == -1).all() and (near[22:] >= 0).all() and (every >= 0).all() and d2[14:22].min() > 1e11


def test_what_is_not_finite_contributes_nothing(pkg):
    S, T = scene_neighbours("source"), scene_neighbours("target")
    pair, _ = pairs_brute(POSE_GENERAL, S["cloud"], S["found"], T["cloud"], T["found"], D_SCENE)
    assert (pair >= 0).sum() > 4000
    none = gicp_numpy([1e200, 0, 0, 0, 0, 0], S["cloud"], S["cov"], T["cloud"], T["cov"], pair)
    assert none["n_pairs"] == 0 and none["n_with_neighbors"] == 0 and none["score"] == 0.0
    assert not none["gradient"].any() and not none["hessian"].any()
    some = gicp_numpy([1e100, 0, 0, 0, 0, 0], S["cloud"], S["cov"], T["cloud"], T["cov"], pair)
    assert some["n_pairs"] == (pair >= 0).sum() and np.isfinite(some["score"]) and some["score"] < -1e199
    assert np.isfinite(some["gradient"]).all() and np.isfinite(some["hessian"]).all()
    far, d2 = pairs_brute([3.5e38, 0, 0, 0, 0, 0], S["cloud"], S["found"], T["cloud"], T["found"], np.inf)
    assert (far == -1).all() and np.isinf(d2).all()


def test_the_loop_converges_under_the_cap(pkg):
    """gicp_align_numpy on the scene under a neighbour cap of 0.8 m, from the scene's guess"""
    s = scene()
    eps = DEFAULTS["covariance_epsilon"]
    S, T = brute("scene-source", 20, 0.8), brute("scene-target", 20, 0.8)
    ref = gicp_align_numpy(pkg, s["ideal"], reg_cov_numpy(S["raw"], eps)[0], S["found"], s["target"], reg_cov_numpy(T["raw"], eps)[0],
                           T["found"], s["guess"])
    print("cap 0.8: %d outer iterations, inner %s, %d pairs" % (ref["outer"], ref["inner"], ref["n_pairs"]))
    assert ref["converged"] and ref["n_pairs"] > 4000
