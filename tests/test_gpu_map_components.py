"""Connected components of the voxel map on the device (ndt_map_components, ndt_map_export_components,
ndt_map_export_labels / _device, ndt_map_label_points / _device, ndt_map_remove_components) against `components_numpy`
and `remove_numpy`, the NumPy restatements of the header's rule in tests/test_map_components_cpu.py (which checks them
against hand-worked cases and scipy.ndimage.label).  Every expectation is an integer and every comparison is ==: labels,
component records, counts and ndt_map_get_info; the survivors of a removal are the table's own records, moved, so the
state export afterwards is compared on its bits.  The restatement always runs on ndt_map_export_state of the very map the
device labelled.
Shapes: two voxels; an 8^3 checkerboard (256 voxels); a one-voxel-wide path of 4096 voxels (16 blocks of slots and more,
diameter = length); the ends of the coordinate range; a 64-slot table whose probe runs cross its end; 20 000 random
voxels in a 48^3 box (fill 0.18, below the face-percolation threshold: hundreds of components of many sizes)."""
import numpy as np
import pytest

from test_gpu_map_levels import assert_level_is_the_rule
from test_gpu_map_target import engine, eval_words, leaf_bytes
from test_map_components_cpu import (COMP_FIELDS, CONNECTIVITIES, LIMIT, components_numpy, map_hash_numpy, pow2_at_least,
                                     remove_numpy, snake_path)
from test_map_state_cpu import filter_state, state_key, states_equal
from test_map_target_cpu import host_transform_f64, voxel_ijk

pytestmark = pytest.mark.gpu

LEAF = 1.0


def centres(ijk, leaf=LEAF):
    """one point per voxel: its centre (exact in f32 for |ijk| < 2^20 at leaf 1 and 0.5)"""
    return ((np.asarray(ijk, np.float64) + 0.5) * leaf).astype(np.float32)


def state_of(ijk, count, leaf=LEAF, moments=False, seed=0):
    """records for ndt_map_import_state: the sums of `count` points at the voxel's centre; moments that are just numbers"""
    ijk = np.asarray(ijk, np.int32).reshape(-1, 3)
    count = np.asarray(count, np.int32).reshape(-1)
    sums = np.zeros((len(ijk), 4), np.float32)
    sums[:, :3] = centres(ijk, leaf) * count[:, None].astype(np.float32)
    mom = np.random.default_rng(seed).normal(size=(len(ijk), 9)) if moments else None
    return dict(leaf=leaf, ijk=ijk, count=count, sums=sums, moments=mom)


def imported(pkg, ijk, count, leaf=LEAF, moments=False, capacity=0):
    ndt = engine(pkg, leaf)
    ndt.mapReset(leaf, initial_capacity=capacity)
    if moments:
        ndt.mapEnableMoments()
    ndt.mapImportState(state_of(ijk, count, leaf, moments))
    return ndt


def added(pkg, ijk, leaf=LEAF, capacity=0, chunks=None):
    """one point per voxel centre through ndt_map_add, in the given chunks"""
    ndt = engine(pkg, leaf)
    ndt.mapReset(leaf, initial_capacity=capacity)
    pts = centres(ijk, leaf)
    at = 0
    for n in (chunks or [len(pts)]):
        if at < len(pts):
            ndt.mapAdd(pts[at:at + n])
        at += n
    assert at >= len(pts)
    return ndt


def outputs(pkg, ndt, connectivity, min_count=1):
    """everything the device reports for one (connectivity, min_count)"""
    info = pkg.mapComponents(ndt, connectivity, min_count)
    lab = pkg.mapExportLabels(ndt, connectivity, min_count)
    comps = pkg.mapExportComponents(ndt, connectivity, min_count)
    return info, lab, comps


def check(pkg, ndt, connectivity, min_count=1, what=""):
    """The device's labelling against the restatement run on ndt_map_export_state of the same map.  Returns (state, cc)."""
    st = ndt.mapExportState()
    cc = components_numpy(st["ijk"], st["count"], connectivity, min_count)
    info, lab, comps = outputs(pkg, ndt, connectivity, min_count)
    assert np.array_equal(cc["ijk"], st["ijk"]) and np.array_equal(lab["ijk"], st["ijk"]), what      # row r is row r
    assert lab["label"].dtype == np.int32 and np.array_equal(lab["label"], cc["label"]), (what, connectivity, min_count)
    assert info == cc["info"], (what, info, cc["info"])
    for k in COMP_FIELDS:
        assert comps[k].dtype == cc["comps"][k].dtype and np.array_equal(comps[k], cc["comps"][k]), (what, k)
    return st, cc


# ---- 1. the smallest maps -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_empty_one_and_two_voxels(pkg, connectivity):
    ndt = engine(pkg, LEAF)
    ndt.mapReset(LEAF)
    info, lab, comps = outputs(pkg, ndt, connectivity)
    assert info == dict(n_components=0, n_voxels_labelled=0, n_voxels_unlabelled=0, largest=-1, largest_n_voxels=0, largest_n_points=0)
    assert len(lab["label"]) == 0 and len(comps["n_voxels"]) == 0
    assert pkg.mapRemoveComponents(ndt, connectivity, min_voxels=5) == dict(n_components=0, n_components_removed=0, n_removed=0,
                                                                           n_points_removed=0)
    labels, k = pkg.mapLabelPoints(ndt, np.zeros((5, 3), np.float32), connectivity=connectivity)
    assert labels.tolist() == [-1] * 5 and k == 0
    ndt.mapAdd(centres([(3, -4, 5)]))
    _, cc = check(pkg, ndt, connectivity, what="one")
    assert cc["info"]["n_components"] == 1
    want = {6: (1, 2, 2, 2), 18: (1, 1, 2, 2), 26: (1, 1, 1, 2)}[connectivity]
    for other, n in zip(((4, -4, 5), (4, -3, 5), (2, -5, 6), (3, -4, 7)), want):              # a face, an edge, a corner, apart
        for first in (0, 1):                                                                  # either one is the root
            pair = [(3, -4, 5), other][::1 if first else -1]
            _, cc = check(pkg, added(pkg, pair), connectivity, what=str(other))
            assert cc["info"]["n_components"] == n, (other, connectivity)


# ---- 2. checkerboard and snake ---------------------------------------------------------------------------------------------
def test_checkerboard(pkg):
    g = np.array([(i, j, k) for k in range(8) for j in range(8) for i in range(8) if (i + j + k) % 2 == 0]) - 3
    ndt = added(pkg, g)
    counts = [check(pkg, ndt, c)[1]["info"]["n_components"] for c in CONNECTIVITIES]
    assert counts == [256, 1, 1]


@pytest.mark.parametrize("capacity", [0, 16])
def test_snake(pkg, capacity):
    path = snake_path(4096) - 9
    chunks = [16, 100, 1000, 2980] if capacity else None
    ndt = added(pkg, path, capacity=capacity, chunks=chunks)
    info = ndt.mapInfo()
    assert info["n_voxels"] == 4096
    if capacity:
        assert info["n_grows"] >= 3 and info["capacity"] == 8192                              # the table has grown several times
    _, cc = check(pkg, ndt, 6, what="snake")
    assert cc["info"]["n_components"] == 1 and cc["info"]["largest_n_voxels"] == 4096
    ndt = added(pkg, np.delete(path, 2048, axis=0), capacity=capacity, chunks=chunks)
    _, cc = check(pkg, ndt, 6, what="cut snake")
    assert cc["info"]["n_components"] == 2 and sorted(cc["comps"]["n_voxels"].tolist()) == [2047, 2048]
    check(pkg, ndt, 26, what="cut snake, corners")


# ---- 3. the ends of the coordinate range -------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_coordinate_range(pkg, connectivity):
    e = LIMIT - 1
    vox = [(e, 0, 0), (-e, 1, 0), (e - 1, 0, 0), (-e, -e, -e), (-e + 1, -e, -e), (0, -e, 5), (0, -e + 1, 5), (7, 7, -e), (7, 7, e),
           (e, e, e), (e, e, e - 1), (-e, 0, 0), (e, -1, 0)]
    ndt = imported(pkg, vox, np.arange(1, len(vox) + 1))
    st, cc = check(pkg, ndt, connectivity, what="range")
    lab = {tuple(v): int(l) for v, l in zip(cc["ijk"].tolist(), cc["label"])}
    # a carry out of the key's i field would join the first pair; the second pair are neighbours
    assert lab[(e, 0, 0)] != lab[(-e, 1, 0)] and lab[(e, 0, 0)] != lab[(-e, 0, 0)] and lab[(e, 0, 0)] == lab[(e - 1, 0, 0)]
    assert lab[(7, 7, -e)] != lab[(7, 7, e)] and lab[(e, e, e)] == lab[(e, e, e - 1)] and lab[(-e, -e, -e)] == 0
    # ... through ndt_map_add as well
    check(pkg, added(pkg, vox, leaf=0.5), connectivity, what="range, added")


# ---- 4. probe runs that cross the end of the table -----------------------------------------------------------------------------
def wrap_voxels(cap=64, tail=3, pairs=6):
    """voxels whose home position is among the last `tail` of a `cap`-slot table, in adjacent pairs: more keys than
    positions there, so some sit behind the table's end, and a neighbour's probe run crosses it"""
    r = np.arange(-30, 31)
    i, j, k = np.meshgrid(r, r, r, indexing="ij")
    ijk = np.stack([i.ravel(), j.ravel(), k.ravel()], 1)
    home = map_hash_numpy(state_key(ijk).astype(np.uint64)) & np.uint64(cap - 1)
    late = {tuple(v) for v in ijk[home >= cap - tail].tolist()}
    out = []
    for v in sorted(late):
        for d in ((1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1), (-1, 1, 1)):
            w = (v[0] + d[0], v[1] + d[1], v[2] + d[2])
            if w in late and v not in out and w not in out and len(out) < 2 * pairs:
                out += [v, w]
    assert len(out) == 2 * pairs
    return np.array(out, np.int64)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_probe_runs_cross_the_end_of_the_table(pkg, connectivity):
    vox = wrap_voxels()
    home = map_hash_numpy(state_key(vox).astype(np.uint64)) & np.uint64(63)
    assert len(vox) == 12 and (home >= 61).all()                                             # 12 keys for 3 positions
    ndt = imported(pkg, vox, np.arange(1, 13), capacity=64)
    assert ndt.mapInfo()["capacity"] == 64
    _, cc = check(pkg, ndt, connectivity, what="wrap")
    assert cc["info"]["n_voxels_labelled"] == 12
    pts = centres(vox)
    labels, k = pkg.mapLabelPoints(ndt, pts, connectivity=connectivity)                       # map_find crosses the end as well
    lab = {tuple(v): int(l) for v, l in zip(cc["ijk"].tolist(), cc["label"])}
    assert labels.tolist() == [lab[tuple(v)] for v in vox.tolist()] and k == 12


# ---- 5. min_count --------------------------------------------------------------------------------------------------------------
def test_min_count_bridge(pkg):
    blob = [(i, j, k) for i in range(3) for j in range(3) for k in range(3)]
    a = np.array(blob)
    b = np.array(blob) + [4, 0, 0]
    bridge = np.array([[3, 1, 1]])
    vox = np.concatenate([a, b, bridge])
    count = np.array([3] * 54 + [1])
    ndt = imported(pkg, vox, count, moments=True)
    _, cc = check(pkg, ndt, 6, 1)
    assert cc["info"]["n_components"] == 1 and cc["info"]["n_voxels_unlabelled"] == 0
    st, cc = check(pkg, ndt, 6, 2)
    at = int(np.flatnonzero((st["ijk"] == [3, 1, 1]).all(1))[0])
    assert cc["info"]["n_components"] == 2 and cc["label"][at] == -1 and cc["info"]["n_voxels_unlabelled"] == 1
    check(pkg, ndt, 26, 4)                                                                    # nothing is eligible
    assert pkg.mapComponents(ndt, 26, 4)["n_components"] == 0
    r = pkg.mapRemoveComponents(ndt, 6, 2, remove_unlabelled=True)
    assert r == dict(n_components=2, n_components_removed=0, n_removed=1, n_points_removed=1)
    keep = np.ones(55, bool)
    keep[at] = False
    assert states_equal(ndt.mapExportState(), filter_state(st, keep))                         # the bridge and nothing else
    _, cc = check(pkg, ndt, 6, 1)
    assert cc["info"]["n_components"] == 2


# ---- 6. the random field ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field():
    rng = np.random.default_rng(2024)
    cells = rng.choice(48 ** 3, 20000, replace=False)
    ijk = np.stack([cells % 48, (cells // 48) % 48, cells // 2304], 1).astype(np.int64) - 20
    count = rng.integers(1, 10, 20000)
    cc = {c: components_numpy(ijk, count, c) for c in CONNECTIVITIES}                        # computed once, shared, left alone
    return dict(ijk=ijk, count=count, cc=cc)


def test_random_field(pkg, field):
    ndt = imported(pkg, field["ijk"], field["count"])
    shuffled = np.random.default_rng(3).permutation(20000)
    other = imported(pkg, field["ijk"][shuffled], field["count"][shuffled], capacity=1 << 16)
    assert ndt.mapInfo()["capacity"] != other.mapInfo()["capacity"]
    for c in CONNECTIVITIES:
        want = field["cc"][c]
        st, cc = check(pkg, ndt, c, what="field")
        assert np.array_equal(cc["label"], want["label"]) and cc["info"] == want["info"]
        info, lab, comps = outputs(pkg, other, c)                                             # another order, another capacity
        assert info == want["info"] and np.array_equal(lab["label"], want["label"]) and np.array_equal(lab["ijk"], want["ijk"])
        for k in COMP_FIELDS:
            assert np.array_equal(comps[k], want["comps"][k]), k
    n6 = field["cc"][6]["info"]["n_components"]
    assert n6 > 300 and len(set(field["cc"][6]["comps"]["n_voxels"].tolist())) > 10           # hundreds, of many sizes
    assert field["cc"][6]["info"]["n_components"] > field["cc"][18]["info"]["n_components"] > field["cc"][26]["info"]["n_components"]
    # min_count on the same map
    check(pkg, ndt, 18, 4, what="field, min_count 4")


def test_size_protocol_and_device_export(pkg, field, hipmem):
    ndt = imported(pkg, field["ijk"][:3000], field["count"][:3000])
    st, cc = check(pkg, ndt, 6)
    C_ = cc["info"]["n_components"]
    import ctypes as C
    L = pkg.lib()
    prm = pkg.MapComponentsParams()
    L.ndt_map_components_default_params(C.byref(prm))
    prm.connectivity = 6
    n = C.c_size_t(0)
    assert L.ndt_map_export_components(ndt._h, C.byref(prm), None, 0, C.byref(n)) == -1 and n.value == C_      # too small: the size
    few = (pkg.MapComponent * 5)()
    assert L.ndt_map_export_components(ndt._h, C.byref(prm), few, 5, C.byref(n)) == -1 and n.value == C_
    assert [few[k].n_voxels for k in range(5)] == cc["comps"]["n_voxels"][:5].tolist()                        # ... and what fits
    assert L.ndt_map_export_labels(ndt._h, C.byref(prm), None, None, 0, C.byref(n)) == -1 and n.value == 3000
    lab = np.full(3000, -7, np.int32)
    assert L.ndt_map_export_labels(ndt._h, C.byref(prm), None, lab.ctypes.data, 3000, C.byref(n)) == 0          # ijk may be NULL
    assert np.array_equal(lab, cc["label"])
    d_ijk, d_lab = hipmem.upload(np.zeros((3000, 3), np.int32)), hipmem.upload(np.zeros(3000, np.int32))
    assert pkg.mapExportLabelsDevice(ndt, d_ijk, d_lab, 3000, connectivity=6) == 3000
    got_ijk, got_lab = np.zeros((3000, 3), np.int32), np.zeros(3000, np.int32)
    assert hipmem.rt.hipMemcpy(got_ijk.ctypes.data, C.c_void_p(d_ijk), got_ijk.nbytes, 2) == 0
    assert hipmem.rt.hipMemcpy(got_lab.ctypes.data, C.c_void_p(d_lab), got_lab.nbytes, 2) == 0
    assert np.array_equal(got_ijk, st["ijk"]) and np.array_equal(got_lab, cc["label"])


# ---- 7. freshness ------------------------------------------------------------------------------------------------------------------
def test_a_labelling_follows_every_change_of_the_map(pkg):
    a = [(i, 0, 0) for i in range(5)]
    b = [(i, 0, 0) for i in range(6, 11)]
    far = [(i, 9, 3) for i in range(4)]
    ndt = added(pkg, a + b + far)
    _, cc = check(pkg, ndt, 6, what="start")
    assert cc["info"]["n_components"] == 3
    ndt.mapAdd(centres([(5, 0, 0)]))                                                          # joins a and b
    _, cc = check(pkg, ndt, 6, what="mapAdd")
    assert cc["info"]["n_components"] == 2 and cc["info"]["largest_n_voxels"] == 11
    assert ndt.mapCrop([-1.0, 8.0, 2.0], [20.0, 10.0, 4.0], remove_inside=True) == 4          # `far` goes
    _, cc = check(pkg, ndt, 6, what="mapCrop")
    assert cc["info"]["n_components"] == 1
    # two rays straight down through the voxel in the middle of the row: it goes, and the row is two pieces again
    r = ndt.mapCarve(np.float32([[5.5, 0.5, -3.5]] * 2), [5.5, 0.5, 8.5], min_misses=2, keep_last=0)
    assert r["n_removed"] == 1
    _, cc = check(pkg, ndt, 6, what="mapCarve")
    assert cc["info"]["n_components"] == 2 and cc["comps"]["n_voxels"].tolist() == [5, 5]


# ---- 8. the points of a cloud -------------------------------------------------------------------------------------------------------
def test_label_points(pkg, field, hipmem):
    import ctypes as C
    leaf = 0.5
    ijk, count = field["ijk"][:6000], field["count"][:6000]
    ndt = imported(pkg, ijk, count, leaf=leaf)
    T = np.eye(4)
    c, s = np.cos(0.3), np.sin(0.3)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [1.25, -2.5, 0.75]
    rng = np.random.default_rng(9)
    inside = centres(ijk[rng.integers(0, 6000, 1500)], leaf) + rng.uniform(-0.24, 0.24, (1500, 3)).astype(np.float32)
    faces = (rng.integers(-40, 60, (600, 3)) * leaf).astype(np.float32)                        # exactly on voxel faces
    anywhere = rng.uniform(-14, 16, (900, 3)).astype(np.float32)                              # occupied or not
    moved_want = np.concatenate([inside, faces, anywhere])
    Ti = np.linalg.inv(T)
    cloud = host_transform_f64(Ti, moved_want)                                                # (about where the pose puts them back)
    special = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [6e5, 0, 0], [0, -6e5, 0], [3e38, 3e38, 3e38]])
    cloud = np.concatenate([cloud, faces, special])                                           # (the faces as they are, too)
    T2 = np.eye(4)
    T2[:3, 3] = [1.5, -2.0, 0.5]                                                              # whole voxels: faces stay faces
    for min_count in (1, 3):
        st, cc = check(pkg, ndt, 18, min_count)
        lab = {tuple(v): int(l) for v, l in zip(cc["ijk"].tolist(), cc["label"])}
        for pose in (T, T2, None):
            with np.errstate(over="ignore", invalid="ignore"):
                moved = cloud if pose is None else host_transform_f64(pose, cloud)
                fin = np.isfinite(cloud).all(1) & np.isfinite(moved).all(1)
                vox = np.floor(np.where(fin[:, None], moved, np.float32(0)) * (np.float32(1.0) / np.float32(leaf)))
                ok = fin & (np.abs(vox) < LIMIT).all(1)
            vox = np.where(ok[:, None], vox, np.float32(0)).astype(np.int64)
            want = np.array([lab.get(tuple(v), -1) if o else -1 for v, o in zip(vox.tolist(), ok)], np.int32)
            got, k = pkg.mapLabelPoints(ndt, cloud, pose=pose, connectivity=18, min_count=min_count)
            assert got.dtype == np.int32 and np.array_equal(got, want) and k == int((want >= 0).sum())
            assert (want[-6:] == -1).all()
            if pose is T:                                                                     # points in eligible, ineligible and empty voxels
                assert (want[:1500] >= 0).sum() > 700 and (want[1500:3000] == -1).sum() > 100 and (want[1500:3000] >= 0).sum() > 3
            if pose is not T:                                                                 # the faces are exactly faces here
                on = moved[3000:3600] / np.float32(leaf)
                assert np.array_equal(on, np.round(on))
            d = [hipmem.upload(np.ascontiguousarray(cloud[:, a])) for a in range(3)]
            d_out = hipmem.upload(np.full(len(cloud), -9, np.int32))
            assert pkg.mapLabelPointsDevice(ndt, d[0], d[1], d[2], len(cloud), d_out, pose=pose, connectivity=18, min_count=min_count) == k
            back = np.zeros(len(cloud), np.int32)
            assert hipmem.rt.hipMemcpy(back.ctypes.data, C.c_void_p(d_out), back.nbytes, 2) == 0
            assert np.array_equal(back, want)                                                 # the host form and the device form agree
    # the same voxels as ndt_map_add finds them: a map made of the moved cloud holds every finite in-range point's voxel
    probe = engine(pkg, leaf)
    probe.mapReset(leaf)
    fin_rows = np.isfinite(host_transform_f64(T, cloud[:-6])).all(1)
    probe.mapAdd(cloud[:-6][fin_rows], pose=T)
    mine = {tuple(v) for v in voxel_ijk(host_transform_f64(T, cloud[:-6][fin_rows]), leaf).tolist()}
    assert {tuple(v) for v in probe.mapExportState()["ijk"].tolist()} == mine
    assert pkg.mapLabelPoints(ndt, np.zeros((0, 3), np.float32), pose=T) [1] == 0             # n = 0 is a no-op


# ---- 9. removal ----------------------------------------------------------------------------------------------------------------------
FILTERS = {
    "min_voxels": dict(min_voxels=3),
    "min_points": dict(min_points=12),
    "keep_largest": dict(keep_largest=5),
    "combined": dict(min_voxels=2, min_points=9, keep_largest=40),
    "with_unlabelled": dict(min_voxels=4, remove_unlabelled=True),
}


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_remove_components(pkg, field, name):
    flt = FILTERS[name]
    min_count = 3 if name == "with_unlabelled" else 1
    ndt = imported(pkg, field["ijk"], field["count"], moments=True, capacity=1 << 12)
    st, cc = check(pkg, ndt, 6, min_count)
    info0 = ndt.mapInfo()
    want = remove_numpy(cc, dict(info0, reset_capacity=1 << 12), **flt)
    assert 0 < want["result"]["n_removed"] < 20000 and want["result"]["n_components_removed"] > 0
    dry = pkg.mapRemoveComponents(ndt, 6, min_count, dry_run=True, **flt)
    assert dry == want["result"] and ndt.mapInfo() == info0 and states_equal(ndt.mapExportState(), st)   # counted, not changed
    got = pkg.mapRemoveComponents(ndt, 6, min_count, **flt)
    print(name, got)
    assert got == want["result"]
    after, info = ndt.mapExportState(), ndt.mapInfo()
    assert states_equal(after, filter_state(st, want["keep"]))                                 # bit for bit, moments included
    assert info == {k: v for k, v in want["info"].items() if k != "reset_capacity"}
    # what is left passes the filter: a second call has nothing to remove and leaves the table untouched
    if "keep_largest" not in flt:
        again = pkg.mapRemoveComponents(ndt, 6, min_count, **flt)
        assert again["n_removed"] == 0 and ndt.mapInfo() == info and states_equal(ndt.mapExportState(), after)
    check(pkg, ndt, 6, min_count, what="after the removal")


def test_remove_components_edges(pkg):
    # two components of equal size: keep_largest = 1 keeps the one with the lower index
    a = [(i, 0, 0) for i in range(4)]
    b = [(i, 0, 5) for i in range(4)]
    c = [(9, 9, 2)]
    ndt = imported(pkg, a + b + c, [2] * 9, moments=True)
    st, cc = check(pkg, ndt, 6)
    assert cc["comps"]["n_voxels"].tolist() == [4, 1, 4]
    info0 = ndt.mapInfo()
    assert pkg.mapRemoveComponents(ndt, 6) == dict(n_components=3, n_components_removed=0, n_removed=0, n_points_removed=0)
    assert ndt.mapInfo() == info0 and states_equal(ndt.mapExportState(), st)                   # nothing to remove: untouched
    r = pkg.mapRemoveComponents(ndt, 6, keep_largest=1)
    assert r == dict(n_components=3, n_components_removed=2, n_removed=5, n_points_removed=10)
    after = ndt.mapExportState()
    assert after["ijk"].tolist() == [list(v) for v in a] and states_equal(after, filter_state(st, st["ijk"][:, 2] == 0))
    info = ndt.mapInfo()
    assert (info["n_voxels"], info["n_points"], info["min_ijk"], info["max_ijk"]) == (4, 8, (0, 0, 0), (3, 0, 0))
    # a filter that removes everything leaves an existing, empty map
    r = pkg.mapRemoveComponents(ndt, 6, min_voxels=5)
    assert r == dict(n_components=1, n_components_removed=1, n_removed=4, n_points_removed=8)
    info = ndt.mapInfo()
    assert info["n_voxels"] == 0 and info["n_points"] == 0 and ndt.mapHasMoments() and len(ndt.mapExportState()["count"]) == 0
    assert pkg.mapComponents(ndt, 6)["n_components"] == 0
    ndt.mapImportState(state_of(a, [1] * 4, moments=True))                                     # ... that goes on as a map
    assert check(pkg, ndt, 6)[1]["info"]["n_components"] == 1


# ---- 10. the rest of the handle -----------------------------------------------------------------------------------------------------
def test_the_rest_of_the_handle_is_left_alone(pkg, S):
    src, tgt, gt, guess = S.two_planes(seed=7, max_points=4000)

    def run(with_calls):
        ndt = engine(pkg, 1.0)
        ndt.mapReset(1.0)
        ndt.mapEnableMoments()
        ndt.mapAdd(tgt)
        ndt.mapAdd(np.float32([[40.5, 40.5, 40.5], [41.5, 40.5, 40.5], [-30.5, 7.5, 2.5]]))    # speckle
        ndt.setInputTarget(tgt)
        ndt.setInputSource(src)
        ndt.putKeyframe(3, src)
        seen = []
        if with_calls:
            lvl = pkg.mapExportStateLevel(ndt, 1)
            seen.append(pkg.mapComponents(ndt, 18))
            pkg.mapExportLabels(ndt, 18)
            pkg.mapExportComponents(ndt, 18)
            pkg.mapLabelPoints(ndt, src, pose=guess)
            assert pkg.mapRemoveComponents(ndt, 18, min_voxels=3, dry_run=True)["n_removed"] >= 3
            assert states_equal(pkg.mapExportStateLevel(ndt, 1), lvl)                          # a labelling is no change of the map
        T = ndt.align(guess)
        fit = ndt.getFitnessScore()
        words = eval_words(pkg, ndt, [0.01, -0.02, 0.03, 0.001, -0.002, 0.003])
        if with_calls:
            r = pkg.mapRemoveComponents(ndt, 18, min_voxels=3)
            assert r["n_removed"] >= 3
            assert_level_is_the_rule(pkg, ndt, 1, "after the removal")                        # re-derived from the smaller map
            assert len(pkg.mapExportStateLevel(ndt, 1)["count"]) < len(lvl["count"])
        h = ndt.getIterationHistory()
        return (np.asarray(T).tobytes(), np.float64(fit).tobytes(), words.tobytes(), leaf_bytes(pkg, ndt), [a.tobytes() for a in h],
                ndt.sourceSize(), ndt.keyframeCount(), ndt.getTiming()["n_eval_launches"], ndt.getGridInfo()["n_target_points"])

    assert run(True) == run(False)
