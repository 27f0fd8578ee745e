"""The voxel map's levels (ndt_map_level_info, ndt_map_export_state_level / _device, ndt_set_target_from_map_level,
ndt_map_coarsen, ndt_map_levels_drop, ndt_align_map_levels) on the device, against
  (A) level_numpy (tests/test_map_levels_cpu.py): the rule of include/ndt_hip.h restated -- np.array_equal on ijk, count,
      the four f32 sums and the nine f64 moments;
  (B) the route the rule names as its equal: ndt_map_import_state of the level's records into an empty map of leaf_L and
      ndt_set_target_from_map_moments there -- leaf bytes and evaluation words, byte for byte;
  (C) the oracle on the concatenation of everything added, at leaf_L: cells, counts and grid geometry exactly on any
      scene; on a scene quantised to multiples of 2^-10 within +-60 m, where every one of the nine f64 sums is exact
      whatever the order, also a map built at leaf_L from the same adds byte for byte and the oracle at the tolerances of
      tests/test_gpu_parity.py (mean 1e-12, covariance 1e-9 / inverse 1e-7 of the largest entry, align 1 mm / 0.1 mrad).
Base shape as tests/test_gpu_map_target.py: 4 scans of 32 x 256 beams, each moved by its pose."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_map_levels_cpu import level_leaf, level_numpy
from test_map_state_cpu import filter_state, states_equal
from test_map_target_cpu import host_transform_f64, voxel_ijk

pytestmark = pytest.mark.gpu

ALIGN_TOL_M, ALIGN_TOL_RAD = 1e-3, 1e-4
INVALID_ARG, NO_TARGET, GRID_OVERFLOW = -1, -4, -6
KW = dict(step_size=0.1, trans_epsilon=1e-4, max_iterations=35)
OFFSET = np.float64([0.05, -0.03, 0.02, 0.01, -0.005, 0.008])
# the basin check's guess: truth + BASIN (x, y, yaw), chosen on the CPU with the oracle (test_align_map_levels_widens_the_basin)
BASIN = np.float64([1.0, 0.5, 0.0, 0.0, 0.0, 0.05])


# ---- helpers (those of tests/test_gpu_map_target.py, copied) ------------------------------------------------------------
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


def code_of(pkg, fn, *a, **k):
    with pytest.raises(pkg.NdtError) as ei:
        fn(*a, **k)
    return ei.value.code


def download(hipmem, ptr, like):
    out = np.zeros_like(like)
    assert hipmem.rt.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0
    return out


def target_print(pkg, ndt, poses6):
    """what a target is, as bytes: geometry, leaves, and the evaluation words at the poses"""
    gi = ndt.getGridInfo()
    geo = tuple(np.asarray(gi[k]).tobytes() for k in ("min_b", "max_b", "div_b")) + (gi["n_cells"], gi["n_leaves"], gi["n_target_points"])
    return geo, leaf_bytes(pkg, ndt), [eval_words(pkg, ndt, p).tobytes() for p in poses6]


def level_map(pkg, leaf, pieces, moments=True, intensity=False, resolution=None, **kw):
    ndt = engine(pkg, leaf if resolution is None else resolution, **kw)
    ndt.mapReset(leaf, with_intensity=intensity)
    if moments:
        ndt.mapEnableMoments()
    for piece in pieces:
        ndt.mapAdd(piece, intensity_column=3 if intensity else None)
    return ndt


def imported_map(pkg, st, moments=True, resolution=None, capacity=0):
    """an empty map of the state's leaf that received the state through mapImportState"""
    ndt = engine(pkg, st["leaf"] if resolution is None else resolution)
    ndt.mapReset(st["leaf"], with_intensity=bool(st.get("with_intensity", False)), initial_capacity=capacity)
    if moments:
        ndt.mapEnableMoments()
    ndt.mapImportState(st)
    return ndt


def assert_level_is_the_rule(pkg, ndt, L, label=""):
    """the level's state against level_numpy of the map's own state, every bit; the info against both"""
    st = ndt.mapExportState()
    want = level_numpy(st, L)
    got = pkg.mapExportStateLevel(ndt, L)
    mom = st["moments"] is not None
    assert got["ijk"].dtype == np.int32 and got["count"].dtype == np.int32 and got["sums"].dtype == np.float32
    assert np.array_equal(got["ijk"], want["ijk"]) and np.array_equal(got["count"], want["count"]), label
    assert np.array_equal(got["sums"].view(np.uint32), want["sums"].view(np.uint32)), label
    if mom:
        assert np.array_equal(got["moments"].view(np.uint64), want["moments"].view(np.uint64)), label
    else:
        assert got["moments"] is None and want["moments"] is None
    assert states_equal(got, want, moments=mom)
    info, base = pkg.mapLevelInfo(ndt, L), ndt.mapInfo()
    m = len(want["count"])
    assert info["n_voxels"] == m and info["n_points"] == int(want["count"].astype(np.int64).sum()) == base["n_points"]
    assert np.float32(info["leaf"]) == level_leaf(base["leaf"], L) == np.float32(got["leaf"])
    assert info["with_intensity"] == base["with_intensity"]
    if m:
        assert info["min_ijk"] == tuple(want["ijk"].min(0)) and info["max_ijk"] == tuple(want["ijk"].max(0))   # tight
        cap = info["capacity"]
        assert cap >= 2 * m and cap & (cap - 1) == 0
    return st, want


@pytest.fixture(scope="module")
def base():
    from slam_sam_amd import replay
    stream = replay.make_stream(n_frames=4, beams=32, cols=256)
    scans = [np.ascontiguousarray(s[:, :3], np.float32) for s, _ in stream]
    poses = [T for _, T in stream]
    moved = [host_transform_f64(T, s) for s, T in zip(scans, poses)]
    cat = np.concatenate(moved)
    assert len(cat) == 32768
    rng = np.random.default_rng(21)
    moved_i = [np.concatenate([m, rng.uniform(0, 255, (len(m), 1)).astype(np.float32)], axis=1) for m in moved]
    # the quantised scene: multiples of 2^-10 within +-60 m -- squares below 2^12 * 2^20 quanta of 2^-20, a few thousand
    # points per voxel at the most: every partial sum of the nine moments is an integer below 2^53 quanta, exact in f64
    q = 2.0 ** -10
    quant = [(np.round(m.astype(np.float64) / q) * q).astype(np.float32) for m in moved]
    quant = [m[(np.abs(m) < 60.0).all(axis=1)] for m in quant]
    assert [len(m) for m in quant] == [7757, 7731, 7707, 7684]
    return dict(scans=scans, poses=poses, moved=moved, moved_i=moved_i, cat=cat, quant=quant, qcat=np.concatenate(quant))


def vehicle_box(base):
    c = base["poses"][3][:3, 3]
    return np.float32(c - [12.0, 9.0, 4.0]), np.float32(c + [12.0, 9.0, 4.0])


def in_level_box(ijk, leaf_l, box_min, box_max):
    """the level voxels a box selects: floor(box * inv_leaf_L) in f32 on both corners, both ends included"""
    lo = voxel_ijk(np.float32(box_min)[None], float(leaf_l))[0]
    hi = voxel_ijk(np.float32(box_max)[None], float(leaf_l))[0]
    return ((ijk >= lo) & (ijk <= hi)).all(axis=1)


# ---- 1. the level's state is the rule, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [0.5, 0.3])
@pytest.mark.parametrize("intensity,moments", [(False, True), (True, True), (False, False), (True, False)])
def test_level_state_equals_the_numpy_rule(pkg, base, hipmem, leaf, intensity, moments):
    ndt = level_map(pkg, leaf, base["moved_i"] if intensity else base["moved"], moments, intensity)
    lo, hi = vehicle_box(base)
    for L in (1, 2, 3):
        st, want = assert_level_is_the_rule(pkg, ndt, L, "leaf %g L %d" % (leaf, L))
        m = len(want["count"])
        assert 256 < m < len(st["count"])                                           # more than one block of level voxels
        if intensity:
            assert float(np.abs(want["sums"][:, 3]).max()) > 0
        else:
            assert not want["sums"][:, 3].any()
        # a box equals the whole level filtered, edge leaves complete
        keep = in_level_box(want["ijk"], level_leaf(leaf, L), lo, hi)
        assert 0 < keep.sum() < m
        boxed = pkg.mapExportStateLevel(ndt, L, lo, hi)
        assert states_equal(boxed, filter_state(want, keep), moments=moments)
    # the device form writes the same records
    L = 2
    want = level_numpy(ndt.mapExportState(), L)
    m = len(want["count"])
    d_ijk, d_cnt = hipmem.upload(np.zeros((m, 3), np.int32)), hipmem.upload(np.zeros(m, np.int32))
    d_sums = hipmem.upload(np.zeros((m, 4), np.float32))
    d_mom = hipmem.upload(np.zeros((m, 9), np.float64)) if moments else None
    assert pkg.mapExportStateLevelDevice(ndt, L, d_ijk, d_cnt, d_sums, d_mom, m) == m
    assert np.array_equal(download(hipmem, d_ijk, want["ijk"]), want["ijk"])
    assert np.array_equal(download(hipmem, d_cnt, want["count"]), want["count"])
    assert np.array_equal(download(hipmem, d_sums, want["sums"]).view(np.uint32), want["sums"].view(np.uint32))
    if moments:
        assert np.array_equal(download(hipmem, d_mom, want["moments"]).view(np.uint64), want["moments"].view(np.uint64))
    else:
        assert code_of(pkg, pkg.mapExportStateLevelDevice, ndt, L, d_ijk, d_cnt, d_sums, d_sums, m) == INVALID_ARG
    keep = in_level_box(want["ijk"], level_leaf(leaf, L), lo, hi)
    assert pkg.mapExportStateLevelDevice(ndt, L, d_ijk, None, None, None, m, lo, hi) == int(keep.sum())
    assert np.array_equal(download(hipmem, d_ijk, want["ijk"])[:keep.sum()], want["ijk"][keep])
    assert code_of(pkg, pkg.mapExportStateLevelDevice, ndt, L, d_ijk, None, None, None, m - 1) == INVALID_ARG   # too small


# ---- 2. hand-made maps ---------------------------------------------------------------------------------------------------
def hand_state(ijk, leaf=0.5, seed=0, count=None):
    rng = np.random.default_rng(seed)
    ijk = np.int32(ijk).reshape(-1, 3)
    n = len(ijk)
    return dict(leaf=leaf, with_intensity=False, ijk=ijk,
                count=np.int32(rng.integers(1, 50, n) if count is None else count),
                sums=np.concatenate([rng.normal(0, 30, (n, 3)), np.zeros((n, 1))], axis=1).astype(np.float32),
                moments=rng.normal(0, 1e3, (n, 9)))


HAND = {
    "negatives": ([[-1, 0, 0], [-2, 0, 0], [-3, 0, 0], [0, -1, -3], [5, -2, -1]], (1, 2)),
    "extremes": ([[2 ** 20 - 1] * 3, [-(2 ** 20 - 1)] * 3, [2 ** 20 - 1, -(2 ** 20 - 1), 0], [2 ** 20 - 2, 2 ** 20 - 1, 2 ** 20 - 1]],
                 (1, 3, 6)),
    "eight_and_one": ([[2 + a, 4 + b, -6 + c] for c in (0, 1) for b in (0, 1) for a in (0, 1)] + [[40, 40, 40]], (1, 2)),
    "single": ([[7, -3, 2]], (1, 4, 6)),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_maps(pkg, name):
    ijk, levels = HAND[name]
    ndt = imported_map(pkg, hand_state(ijk, seed=len(ijk)))
    for L in levels:
        st, want = assert_level_is_the_rule(pkg, ndt, L, "%s L %d" % (name, L))
        if name == "negatives" and L == 1:
            assert [-2, 0, 0] in want["ijk"].tolist() and [-1, 0, 0] in want["ijk"].tolist() and [0, -1, -2] in want["ijk"].tolist()
            assert len(want["count"]) == 4                                            # -1 and -2 share -1; -3 goes to -2
        if name == "extremes" and L == 1:
            assert want["ijk"].max() == 2 ** 19 - 1 and want["ijk"].min() == -(2 ** 19)
        if name == "eight_and_one" and L == 1:
            assert len(want["count"]) == 2 and int(want["count"][0]) == int(st["count"][:8].sum())
        if name == "single":
            assert len(want["count"]) == 1 and states_equal(filter_state(want, [0]), dict(st, ijk=st["ijk"] >> L))


def test_more_level_voxels_than_a_block_and_a_tile(pkg):
    rng = np.random.default_rng(4)
    ijk = np.unique(rng.integers(-40, 40, (30000, 3)), axis=0)
    ndt = imported_map(pkg, hand_state(ijk, seed=1), capacity=64)
    for L in (1, 2, 3):
        _, want = assert_level_is_the_rule(pkg, ndt, L)
        children = np.bincount(np.unique(ijk >> L, axis=0, return_inverse=True)[1].ravel())
        assert len(children) == len(want["count"])
        if L == 1:
            assert len(children) > 4096 and int(children.max()) >= 3
        if L == 2:
            assert len(children) > 1024 and int(children.max()) >= 8                  # more than one export tile (4 x 256)


def test_empty_map_and_count_overflow(pkg, base):
    ndt = engine(pkg, 1.0)
    assert code_of(pkg, pkg.mapLevelInfo, ndt, 1) == INVALID_ARG                    # no map
    assert code_of(pkg, pkg.mapCoarsen, ndt, 1) == INVALID_ARG
    ndt.mapReset(0.5)
    ndt.mapEnableMoments()
    for L in (0, 1, 6):
        info = pkg.mapLevelInfo(ndt, L)
        assert info["n_voxels"] == 0 and info["n_points"] == 0 and np.float32(info["leaf"]) == level_leaf(0.5, L)
        assert len(pkg.mapExportStateLevel(ndt, L)["count"]) == 0
    for bad in (-1, 7):
        assert code_of(pkg, pkg.mapLevelInfo, ndt, bad) == INVALID_ARG
        assert code_of(pkg, pkg.mapExportStateLevel, ndt, bad) == INVALID_ARG
        assert code_of(pkg, pkg.setInputTargetFromMapLevel, ndt, bad) == INVALID_ARG
        assert code_of(pkg, pkg.mapCoarsen, ndt, bad) == INVALID_ARG
    ndt.setParams(resolution=1.0)
    assert code_of(pkg, pkg.setInputTargetFromMapLevel, ndt, 1) == NO_TARGET         # an empty map
    huge = engine(pkg, 1.0)                                                          # leaf * 2 is not finite
    huge.mapReset(3.0e38)
    assert code_of(pkg, pkg.mapLevelInfo, huge, 1) == INVALID_ARG
    # two children of 2^30 points each: the level is refused as a whole; map and target are as they were
    ndt = engine(pkg, 1.0)
    ndt.setInputTarget(base["cat"])
    ndt.setInputSource(base["scans"][3])
    p = [0.1, 0.2, 0.0, 0.0, 0.0, 0.01]
    ndt.mapReset(0.5)
    ndt.mapEnableMoments()
    st = hand_state([[0, 0, 0], [1, 0, 0], [9, 9, 9]], count=[2 ** 30, 2 ** 30, 5])
    ndt.mapImportState(st)
    before = target_print(pkg, ndt, [p])
    assert code_of(pkg, pkg.mapLevelInfo, ndt, 1) == GRID_OVERFLOW
    assert code_of(pkg, pkg.mapExportStateLevel, ndt, 2) == GRID_OVERFLOW
    assert code_of(pkg, pkg.setInputTargetFromMapLevel, ndt, 1) == GRID_OVERFLOW
    assert code_of(pkg, pkg.mapCoarsen, ndt, 1) == GRID_OVERFLOW
    assert target_print(pkg, ndt, [p]) == before
    after = ndt.mapExportState()
    assert states_equal(after, dict(st, ijk=after["ijk"])) and ndt.mapInfo()["leaf"] == 0.5
    ndt.mapCrop([-0.1, -0.1, -0.1], [0.4, 0.4, 0.4], remove_inside=True)              # one of the two goes: the level stands
    assert_level_is_the_rule(pkg, ndt, 1)


# ---- 3. the level target is the target of the imported level -----------------------------------------------------------
@pytest.mark.parametrize("leaf,L", [(0.5, 1), (0.5, 2), (0.3, 2)])
def test_level_target_is_the_target_of_the_imported_level(pkg, O, base, leaf, L):
    leaf_l = float(level_leaf(leaf, L))
    src = base["scans"][3]
    p_gt = O.matrix_to_pose(base["poses"][3])
    poses6 = [p_gt, p_gt + OFFSET]
    a = level_map(pkg, leaf, base["moved"], resolution=leaf_l)
    b = imported_map(pkg, pkg.mapExportStateLevel(a, L))
    assert np.float32(b.mapInfo()["leaf"]) == np.float32(leaf_l)
    for ndt in (a, b):
        ndt.setInputSource(src)
    for box in ((None, None), vehicle_box(base)):
        pkg.setInputTargetFromMapLevel(a, L, *box)
        b.setInputTargetFromMapMoments(*box)
        pa, pb = target_print(pkg, a, poses6), target_print(pkg, b, poses6)
        assert pa[0][4] > 20 and pa == pb, (leaf, L, box)
    assert pa[0][5] < len(base["cat"])                                               # the box holds a part of the map
    # refusals leave the target as it was: a resolution that is not the level's leaf, no moments
    assert code_of(pkg, pkg.setInputTargetFromMapLevel, a, L + 1) == INVALID_ARG
    assert code_of(pkg, pkg.setInputTargetFromMapLevel, a, 0) == INVALID_ARG
    assert code_of(pkg, pkg.setInputTargetFromMapLevel, a, L, [5000.0, 5000.0, 0.0], [5010.0, 5010.0, 9.0]) == NO_TARGET
    assert target_print(pkg, a, poses6) == pa
    plain = level_map(pkg, leaf, base["moved"][:1], moments=False, resolution=leaf_l)
    assert code_of(pkg, pkg.setInputTargetFromMapLevel, plain, L) == INVALID_ARG


# ---- 4. against the points -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf,L", [(0.5, 1), (0.5, 2), (0.3, 1), (0.3, 3)])
def test_level_target_holds_the_oracles_cells_on_the_concatenation(pkg, O, base, leaf, L):
    """membership is exact: cells, counts and grid geometry; the values differ by summation order and are not compared"""
    leaf_l = float(level_leaf(leaf, L))
    cat = base["cat"]
    grid = O.Grid(cat, oracle_params(O, leaf_l))
    OL = grid.export()
    ndt = level_map(pkg, leaf, base["moved"], resolution=leaf_l)
    pkg.setInputTargetFromMapLevel(ndt, L)
    assert_grid_matches(ndt.getGridInfo(), grid, len(cat))
    Lv = ndt.getLeaves()
    assert len(OL["cell"]) > 50 and np.array_equal(Lv["cell"], OL["cell"]) and np.array_equal(Lv["count"], OL["count"])


@pytest.mark.parametrize("leaf,L", [(0.5, 1), (0.5, 2)])
def test_quantised_scene_level_equals_the_map_built_at_the_coarse_leaf(pkg, O, base, leaf, L):
    leaf_l = float(level_leaf(leaf, L))
    qcat, src = base["qcat"], base["scans"][3]
    p_gt = O.matrix_to_pose(base["poses"][3])
    poses6 = [p_gt, p_gt + OFFSET]
    a = level_map(pkg, leaf, base["quant"], resolution=leaf_l)
    c = level_map(pkg, leaf_l, base["quant"])
    la, lc = pkg.mapExportStateLevel(a, L), c.mapExportState()
    assert np.array_equal(la["ijk"], lc["ijk"]) and np.array_equal(la["count"], lc["count"])
    assert np.array_equal(la["moments"].view(np.uint64), lc["moments"].view(np.uint64))   # exact sums: any order, same bits
    for ndt in (a, c):
        ndt.setInputSource(src)
    for box in ((None, None), vehicle_box(base)):
        pkg.setInputTargetFromMapLevel(a, L, *box)
        pkg.setInputTargetFromMapLevel(c, 0, *box)
        assert target_print(pkg, a, poses6) == target_print(pkg, c, poses6)
    grid = O.Grid(qcat, oracle_params(O, leaf_l))
    pkg.setInputTargetFromMapLevel(a, L)
    assert_grid_matches(a.getGridInfo(), grid, len(qcat))
    assert_leaves_match(a.getLeaves(), grid.export(), 1e-9, "level %d of leaf %g vs oracle at %g" % (L, leaf, leaf_l))


# ---- 5. staleness --------------------------------------------------------------------------------------------------------
def test_a_level_follows_every_change_of_the_map(pkg, base):
    leaf = 0.5
    ndt = level_map(pkg, leaf, base["moved"][:2])
    other = level_map(pkg, leaf, base["moved"][3:])
    seen = []

    def check(what):
        for L in (1, 2):
            _, want = assert_level_is_the_rule(pkg, ndt, L, what)
        seen.append((what, len(want["count"]), int(want["count"].astype(np.int64).sum())))
        return want

    first = check("start")
    again = pkg.mapExportStateLevel(ndt, 2)                                           # cached: the same records
    assert states_equal(again, first)
    ndt.mapAdd(base["moved"][2])
    check("mapAdd")
    ndt.mapImportState(other.mapExportState())
    check("mapImportState")
    c = base["poses"][3][:3, 3]
    assert ndt.mapCrop(c - [30.0, 30.0, 10.0], c + [30.0, 30.0, 10.0]) > 0
    check("mapCrop")
    r = ndt.mapCarve(base["scans"][3], [0.0, 0.0, 0.0], pose=base["poses"][3], min_misses=1, keep_last=0)
    print("carve:", r)
    check("mapCarve")
    T = np.eye(4)
    T[:3, 3] = [0.37, -0.21, 0.11]
    pkg.mapTransform(ndt, T)
    check("mapTransform")
    pkg.mapLevelsDrop(ndt)
    check("mapLevelsDrop")
    print(seen)
    assert len({s[1:] for s in seen}) >= 4                                            # the changes were changes
    # a map without moments that gets them: the level has none before and has them after
    late = engine(pkg, leaf)
    late.mapReset(leaf)
    assert pkg.mapExportStateLevel(late, 1)["moments"] is None
    late.mapEnableMoments()
    late.mapAdd(base["moved"][0])
    assert_level_is_the_rule(pkg, late, 1)


# ---- 6. mapCoarsen ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf,L", [(0.5, 1), (0.3, 2)])
def test_coarsen_makes_the_map_its_level(pkg, base, leaf, L):
    leaf_l = float(level_leaf(leaf, L))
    ndt = level_map(pkg, leaf, base["moved"][:3])
    before, level = ndt.mapInfo(), pkg.mapExportStateLevel(ndt, L)
    linfo = pkg.mapLevelInfo(ndt, L)
    pkg.mapCoarsen(ndt, 0)                                                            # the map itself: nothing happens
    assert ndt.mapInfo() == before
    pkg.mapCoarsen(ndt, L)
    info = ndt.mapInfo()
    assert np.float32(info["leaf"]) == np.float32(leaf_l)
    assert states_equal(ndt.mapExportState(), level)
    for k in ("n_points", "n_points_dropped", "n_adds", "n_grows", "with_intensity"):
        assert info[k] == before[k], k
    for k in ("n_voxels", "min_ijk", "max_ijk", "capacity"):
        assert info[k] == linfo[k], k
    assert ndt.mapHasMoments()
    # a later add continues as on a map of that leaf: the same as importing the level into such a map and adding there
    ref = imported_map(pkg, level)
    for m in (ndt, ref):
        m.mapAdd(base["moved"][3])
    assert states_equal(ndt.mapExportState(), ref.mapExportState())
    assert ndt.mapInfo()["n_adds"] == before["n_adds"] + 1
    assert_level_is_the_rule(pkg, ndt, 1)                                             # ... and it has levels of its own
    ndt.setParams(resolution=leaf_l)
    ndt.setInputTargetFromMapMoments()                                                # the coarsened map is a target as it is
    assert ndt.getGridInfo()["n_leaves"] > 20


# ---- 7. alignMapLevels -----------------------------------------------------------------------------------------------------
def params_of(pkg, ndt):
    p = pkg.Params()
    assert pkg.lib().ndt_get_params(ndt._h, C.byref(p)) == 0
    return bytes(p)


STRIP = ("ms_total", "ms_device")


def result_bits(d):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in d.items() if k not in STRIP}


def test_align_map_levels_is_the_sequence_made_by_hand(pkg, O, base):
    leaf = 0.5
    src = base["scans"][3]
    guess = O.pose_to_matrix(O.matrix_to_pose(base["poses"][3]) + [0.3, -0.2, 0.05, 0.0, 0.0, 0.02])
    steps = [(2, 20, 0.2), (1, 0, 0.0), (0, 0, 0.0)]
    half = np.float32([40.0, 40.0, 10.0])
    p_eval = O.matrix_to_pose(base["poses"][3])
    for he in (None, half):
        a = level_map(pkg, leaf, base["moved"])
        b = level_map(pkg, leaf, base["moved"])
        for ndt in (a, b):
            ndt.setInputSource(src)
        saved = params_of(pkg, a)
        got = pkg.alignMapLevels(a, steps, guess, half_extent=he)
        assert params_of(pkg, a) == saved == params_of(pkg, b)                        # restored
        want, cur = [], guess
        for level, iters, step in steps:
            b.setParams(resolution=float(level_leaf(leaf, level)), max_iterations=iters or KW["max_iterations"],
                        step_size=step or KW["step_size"])
            if he is None:
                pkg.setInputTargetFromMapLevel(b, level)
            else:
                t = np.float32(cur[:3, 3])
                pkg.setInputTargetFromMapLevel(b, level, t - he, t + he)
            b.align(cur)
            r = b.getResult()
            want.append(r)
            cur = r["T"]
        b.setParams(resolution=leaf, **KW)
        assert len(got) == 3
        for g, w in zip(got, want):
            gb, wb = result_bits(g), result_bits(w)
            for k in wb:
                if k in gb:
                    assert gb[k] == wb[k], k
            assert g["T"].tobytes() == np.asarray(w["T"], np.float64).tobytes()
        # the last step ran at the caller's own resolution: its target is the handle's target
        assert target_print(pkg, a, [p_eval]) == target_print(pkg, b, [p_eval])
        assert a.getGridInfo()["n_leaves"] > 100
    # a refusal in the middle of the sequence (level 7): its code, the parameters restored, the map as it was
    st = a.mapExportState()
    assert code_of(pkg, pkg.alignMapLevels, a, [2, 7, 0], guess) == INVALID_ARG
    assert params_of(pkg, a) == saved and states_equal(a.mapExportState(), st)
    res = (pkg.Result * 3)()
    arr = (pkg.MapLevelStep * 3)()
    arr[0].level, arr[1].level, arr[2].level = 2, 7, 0
    g16 = np.ascontiguousarray(np.asarray(guess, np.float32).T).ravel()
    assert pkg.lib().ndt_align_map_levels(a._h, arr, 3, None, g16.ctypes.data_as(C.POINTER(C.c_float)), res) == INVALID_ARG
    first = pkg.result_to_dict(res[0])
    assert first["iterations"] > 0 and first["T"][3, 3] == 1.0 and res[1].iterations == 0 and res[2].iterations == 0
    # (the earlier result stays written, the later ones are untouched)
    assert params_of(pkg, a) == saved
    assert code_of(pkg, pkg.alignMapLevels, engine(pkg, leaf), [1, 0], guess) == INVALID_ARG   # no map


@pytest.fixture(scope="module")
def quantised_oracle(O, base):
    """the oracle's grids on the quantised concatenation at 2.0, 1.0 and 0.5 m, shared by the two tests below"""
    return {L: O.Grid(base["qcat"], oracle_params(O, float(level_leaf(0.5, L)))) for L in (2, 1, 0)}


def test_align_map_levels_agrees_with_the_oracle_step_by_step(pkg, O, S, base, quantised_oracle):
    leaf = 0.5
    src, T_gt = base["scans"][3], base["poses"][3]
    guess = O.pose_to_matrix(O.matrix_to_pose(T_gt) + [0.3, -0.2, 0.05, 0.0, 0.0, 0.02])
    ndt = level_map(pkg, leaf, base["quant"])
    ndt.setInputSource(src)
    got = pkg.alignMapLevels(ndt, [2, 1, 0], guess)
    cur = guess
    for L, g in zip((2, 1, 0), got):
        r = quantised_oracle[L].align(src, cur)
        dt, dr = S.pose_error(g["T"], r["T"])
        print("level %d: device vs oracle %.3e m %.3e rad, %d / %d iterations" % (L, dt, dr, g["iterations"], r["iterations"]))
        assert g["converged"] and dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD, (L, dt, dr)
        cur = g["T"]                                                                  # the same three aligns: each from the device's guess


def test_align_map_levels_widens_the_basin(pkg, O, S, base, quantised_oracle):
    """From truth + (1.0 m, 0.5 m, 0, 0, 0, 0.05 rad) on the quantised scene (leaf 0.5, scan 3 as the source), chosen on the
    CPU with the oracle: the oracle's fine-only align ends 1.175 m from truth (converged after 12 iterations, in a wrong
    minimum), the oracle's levels [2, 1, 0] end 0.0110 m, 0.0040 m and 0.0023 m from it.  The device does the same on both
    counts: > 0.5 m fine-only, < 0.05 m through the levels."""
    leaf = 0.5
    src, T_gt = base["scans"][3], base["poses"][3]
    guess = O.pose_to_matrix(O.matrix_to_pose(T_gt) + BASIN)
    o_fine = S.pose_error(quantised_oracle[0].align(src, guess)["T"], T_gt)[0]
    cur = guess
    for L in (2, 1, 0):
        cur = quantised_oracle[L].align(src, cur)["T"]
    o_levels = S.pose_error(cur, T_gt)[0]
    ndt = level_map(pkg, leaf, base["quant"])
    ndt.setInputSource(src)
    d_fine = S.pose_error(pkg.alignMapLevels(ndt, [0], guess)[0]["T"], T_gt)[0]
    d_levels = S.pose_error(pkg.alignMapLevels(ndt, [2, 1, 0], guess)[-1]["T"], T_gt)[0]
    print("fine only: oracle %.4f m device %.4f m; levels [2, 1, 0]: oracle %.4f m device %.4f m" % (o_fine, d_fine, o_levels, d_levels))
    assert o_fine > 0.5 and o_levels < 0.05                                           # the premise, as the docstring states it
    assert d_fine > 0.5 and d_levels < 0.05


# ---- 8. untouched state ----------------------------------------------------------------------------------------------------
def test_level_calls_leave_the_rest_of_the_handle_alone(pkg, base, hipmem):
    leaf = 1.0
    ndt = engine(pkg, leaf)
    ndt.setInputTarget(base["cat"])
    ndt.setInputSource(base["scans"][3])
    ndt.putKeyframe(7, base["scans"][0])
    T = ndt.align(base["poses"][3])
    ndt.mapReset(0.5)
    ndt.mapEnableMoments()
    for m in base["moved"]:
        ndt.mapAdd(m)

    def state():
        h = ndt.getIterationHistory()
        return (leaf_bytes(pkg, ndt), ndt.sourceSize(), [a.tobytes() for a in h], ndt.getTiming()["n_eval_launches"],
                ndt.keyframeCount(), ndt.getFinalTransformation().tobytes(), params_of(pkg, ndt))

    before = state()
    map_before = ndt.mapExportState()
    pkg.mapLevelInfo(ndt, 1)
    assert state() == before
    pkg.mapExportStateLevel(ndt, 2)
    assert state() == before
    d = hipmem.upload(np.zeros(4 * ndt.mapInfo()["n_voxels"], np.int32))
    pkg.mapExportStateLevelDevice(ndt, 1, d, None, None, None, ndt.mapInfo()["n_voxels"])
    assert state() == before
    pkg.mapLevelsDrop(ndt)
    assert state() == before
    assert code_of(pkg, pkg.setInputTargetFromMapLevel, ndt, 2) == INVALID_ARG       # resolution 1.0 is level 1's leaf
    assert state() == before and states_equal(ndt.mapExportState(), map_before)
    assert np.array_equal(ndt.align(base["poses"][3]), T)
    before = state()
    pkg.mapCoarsen(ndt, 1)
    assert state() == before
    assert np.array_equal(ndt.align(base["poses"][3]), T)


def test_level_zero_is_the_map_itself(pkg, O, base, hipmem):
    leaf = 0.5
    a = level_map(pkg, leaf, base["moved"])
    b = level_map(pkg, leaf, base["moved"])
    assert pkg.mapLevelInfo(a, 0) == b.mapInfo()
    lo, hi = vehicle_box(base)
    for box in ((None, None), (lo, hi)):
        assert states_equal(pkg.mapExportStateLevel(a, 0, *box), b.mapExportState(*box))
    n = b.mapInfo()["n_voxels"]
    bufs = [[hipmem.upload(np.zeros((n, 3), np.int32)), hipmem.upload(np.zeros(n, np.int32)),
             hipmem.upload(np.zeros((n, 4), np.float32)), hipmem.upload(np.zeros((n, 9), np.float64))] for _ in range(2)]
    assert pkg.mapExportStateLevelDevice(a, 0, *bufs[0], n) == b.mapExportStateDevice(*bufs[1], n) == n
    for pa, pb, like in zip(bufs[0], bufs[1], (np.zeros((n, 3), np.int32), np.zeros(n, np.int32), np.zeros((n, 4), np.float32),
                                               np.zeros((n, 9), np.float64))):
        assert download(hipmem, pa, like).tobytes() == download(hipmem, pb, like).tobytes()
    p = O.matrix_to_pose(base["poses"][3]) + OFFSET
    for ndt in (a, b):
        ndt.setInputSource(base["scans"][3])
    for box in ((None, None), (lo, hi)):
        pkg.setInputTargetFromMapLevel(a, 0, *box)
        b.setInputTargetFromMapMoments(*box)
        assert target_print(pkg, a, [p]) == target_print(pkg, b, [p])


# ---- 9. the C++ adapter ----------------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, tmp_path):
    """tests/cpp/test_map_levels.cpp against the API mocks, built with the g++ line tests/cpp/Makefile uses for them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "tests", "cpp")
    exe = str(tmp_path / "test_map_levels")
    lib = os.path.join(root, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(root, "include", "compat"), "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(d, "test_map_levels.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "map levels: PASS" in p.stdout
