"""The voxel map bounded, kept and combined (ndt_map_crop, ndt_map_export_state, ndt_map_import_state) against the NumPy
yardsticks of tests/test_map_state_cpu.py: `mapstate_numpy` / `continue_numpy` (per voxel sequential f32 sums and f64
moments in input order, which that file shows to be the un-divided form of the yardsticks the project already trusts) and
`merge_numpy` (old + record per field, one rounding).  Every comparison of ijk, counts, sums and moments is
np.array_equal on the bits: both sides do the same operations in the same order, so no tolerance is needed.  The one
comparison with the oracle (a target made from a cropped map) uses the leaf tolerances of tests/test_gpu_map_target.py.
Base shape: that file's -- 4 scans of 32 x 256 beams (32 768 points), each moved by its pose, leaf 1.0 and 0.5 -- with
the box c +- [12, 9, 4] around the last pose.  The box holds 20 492 of the 32 768 points and, of the voxels with three
points or more (the ones that can become leaves), 552 of 1 625 at leaf 1.0 and 1 164 of 2 185 at leaf 0.5: at least a
quarter on each side, which `base` asserts.  Of ALL occupied voxels it holds 610 of 4 760 and 1 939 of 9 377 (the far
field is mostly voxels of one or two points), fewer than a quarter; `base` asserts at least 500 voxels on each side."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_map_target import (assert_grid_matches, assert_leaves_match, code_of, engine, eval_words, in_box, leaf_bytes,
                                 moment_cases, oracle_params)
from test_map_carve_cpu import DEFAULTS, SCENE_LEAF, carve_numpy, carve_scene, result_of
from test_map_state_cpu import continue_numpy, filter_state, mapstate_numpy, merge_numpy, state_key, states_equal
from test_map_target_cpu import host_transform_f64, voxel_ijk

pytestmark = pytest.mark.gpu

INVALID_ARG, GRID_OVERFLOW = -1, -6
LEAVES = (1.0, 0.5)


def build(pkg, leaf, pieces, poses=None, capacity=0, moments=True, intensity_column=None, **kw):
    ndt = engine(pkg, leaf, **kw)
    ndt.mapReset(leaf, with_intensity=intensity_column is not None, initial_capacity=capacity)
    if moments:
        ndt.mapEnableMoments()
    for k, piece in enumerate(pieces):
        ndt.mapAdd(piece, intensity_column=intensity_column, pose=None if poses is None else poses[k])
    return ndt


def box_mask(ijk, leaf, box_min, box_max):
    """the voxels inside the box: the f32 floor of a point's voxel on both corners, both ends included"""
    lo = voxel_ijk(np.float32(box_min)[None], leaf)[0]
    hi = voxel_ijk(np.float32(box_max)[None], leaf)[0]
    return ((ijk >= lo) & (ijk <= hi)).all(axis=1)


def pow2_at_least(v):
    c = 64
    while c < v:
        c <<= 1
    return c


def export_bits(ndt):
    out, cnt = ndt.mapExport(with_counts=True)
    return np.ascontiguousarray(out, np.float32).view(np.uint32).copy(), cnt.copy()


@pytest.fixture(scope="module")
def base(pkg):
    from slam_sam_amd import replay
    stream = replay.make_stream(n_frames=4, beams=32, cols=256)
    scans = [np.ascontiguousarray(s[:, :3], np.float32) for s, _ in stream]
    poses = [T for _, T in stream]
    moved = [host_transform_f64(T, s) for s, T in zip(scans, poses)]
    cat = np.concatenate(moved)
    assert len(cat) == 32768
    c = poses[3][:3, 3]
    box = (c - [12.0, 9.0, 4.0], c + [12.0, 9.0, 4.0])
    whole, first, second = {}, {}, {}
    for leaf in LEAVES:
        whole[leaf] = mapstate_numpy(cat, leaf)
        first[leaf] = mapstate_numpy(np.concatenate(moved[:2]), leaf)
        second[leaf] = mapstate_numpy(np.concatenate(moved[2:]), leaf)
        st = whole[leaf]
        inside = box_mask(st["ijk"], leaf, *box)
        dense = st["count"] >= 3
        pts_in = int(st["count"][inside].sum())
        print("leaf %.1f: the box holds %d of %d occupied voxels, %d of %d with >= 3 points, %d of %d points"
              % (leaf, inside.sum(), len(inside), (inside & dense).sum(), dense.sum(), pts_in, len(cat)))
        for a, n in (((inside & dense).sum(), dense.sum()), (pts_in, len(cat))):
            assert 4 * a >= n and 4 * (n - a) >= n                                  # a quarter on each side
        assert inside.sum() >= 500 and (~inside).sum() >= 500
    return dict(scans=scans, poses=poses, moved=moved, cat=cat, box=box, whole=whole, first=first, second=second)


# ---- 1. the exported state is the yardstick -----------------------------------------------------------------------------
STATE_CASES = ["poses-1.0", "poses-0.5", "nomoments", "intensity", "grown", "crowded", "nonfinite"]


@pytest.mark.parametrize("name", STATE_CASES)
def test_state_equals_the_yardstick(pkg, base, name):
    leaf, moments, icol, inten = 1.0, True, None, None
    if name.startswith("poses"):
        leaf = float(name.split("-")[1])
        pieces, poses, cap, seen = base["scans"], base["poses"], 0, base["cat"]
        want = base["whole"][leaf]
    elif name == "nomoments":
        pieces, poses, cap, seen = base["moved"], None, 0, base["cat"]
        moments, want = False, base["whole"][leaf]
    elif name == "intensity":
        rng = np.random.default_rng(3)
        inten = rng.uniform(0, 255, len(base["cat"])).astype(np.float32)
        seen = base["cat"]
        pieces = np.array_split(np.concatenate([seen, inten[:, None]], axis=1), 4)
        poses, cap, icol = None, 0, 3
        want = mapstate_numpy(seen, leaf, inten)
        assert want["sums"][:, 3].any()
    else:
        pieces, poses, cap, seen = moment_cases(base, name)
        want = mapstate_numpy(seen, leaf)
    ndt = build(pkg, leaf, pieces, poses, cap, moments=moments, intensity_column=icol)
    st = ndt.mapExportState()
    assert st["leaf"] == np.float32(leaf) and st["with_intensity"] == (icol is not None)
    assert st["ijk"].dtype == np.int32 and st["count"].dtype == np.int32 and st["sums"].dtype == np.float32
    assert (st["moments"] is None) == (not moments)
    assert states_equal(st, want, moments=moments)
    info = ndt.mapInfo()
    assert info["n_voxels"] == len(want["count"]) and info["n_points"] == int(want["count"].sum())
    if name == "grown":
        assert info["n_grows"] >= 1
    if name == "crowded":
        assert int(st["count"].max()) == 5000
    if name == "nonfinite":
        assert info["n_points_dropped"] == 300
    # the box form: the yardstick filtered by the box -- the base box where it splits the map, and the middle half of
    # the map's own extent
    lo, hi = want["ijk"].min(0), want["ijk"].max(0)
    quarter = (hi - lo) // 4
    boxes = [((lo + quarter + 0.5) * leaf, (hi - quarter + 0.5) * leaf)]
    if seen is base["cat"]:
        boxes.append(base["box"])
    for bmin, bmax in boxes:
        keep = box_mask(want["ijk"], leaf, bmin, bmax)
        assert 0 < keep.sum() < len(keep)
        assert states_equal(ndt.mapExportState(bmin, bmax), filter_state(want, keep), moments=moments)
    assert len(ndt.mapExportState([1.0, 1.0, 1.0], [2.0, 0.0, 2.0])["count"]) == 0            # an empty box: nothing, NDT_OK
    assert states_equal(ndt.mapExportState(), want, moments=moments)                          # the map is unchanged
    # too small a cap: INVALID_ARG naming the size, the first `cap` records written
    L, n = pkg.lib(), len(want["count"])
    m = C.c_size_t(0)
    part = np.full((n - 1, 3), -7, np.int32)
    assert L.ndt_map_export_state(ndt._h, None, None, part.ctypes.data, None, None, None, n - 1, C.byref(m)) == INVALID_ARG
    assert m.value == n and str(n) in L.ndt_last_error(ndt._h).decode()
    assert np.array_equal(part, want["ijk"][:n - 1])
    if not moments:                                                                           # moments9 on a map without
        mom = np.zeros((n, 9))
        assert L.ndt_map_export_state(ndt._h, None, None, None, None, None, mom.ctypes.data, n, C.byref(m)) == INVALID_ARG
        assert not mom.any()


# ---- 2. a crop keeps exactly the rest ---------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [0, 64])
@pytest.mark.parametrize("remove_inside", [0, 1])
@pytest.mark.parametrize("leaf", LEAVES)
def test_crop_keeps_exactly_the_rest(pkg, base, leaf, remove_inside, capacity):
    ndt = build(pkg, leaf, base["scans"], base["poses"], capacity)
    before, info0 = ndt.mapExportState(), ndt.mapInfo()
    assert states_equal(before, base["whole"][leaf])
    xyz0, cnt0 = export_bits(ndt)
    reset_cap = pow2_at_least(capacity) if capacity else 1 << 18
    inside = box_mask(before["ijk"], leaf, *base["box"])
    keep = ~inside if remove_inside else inside
    kept = int(keep.sum())
    assert ndt.mapCrop(*base["box"], remove_inside=bool(remove_inside)) == len(keep) - kept
    assert states_equal(ndt.mapExportState(), filter_state(before, keep))
    info = ndt.mapInfo()
    assert info["n_voxels"] == kept and info["n_points"] == int(before["count"][keep].sum())
    assert info["min_ijk"] == tuple(before["ijk"][keep].min(0)) and info["max_ijk"] == tuple(before["ijk"][keep].max(0))   # tight
    assert info["capacity"] == max(pow2_at_least(2 * kept), reset_cap)
    if capacity:
        assert info["capacity"] < info0["capacity"]                                            # (the grown table shrank)
    for k in ("n_points_dropped", "n_adds", "n_grows", "leaf", "with_intensity"):
        assert info[k] == info0[k], k
    xyz, cnt = export_bits(ndt)
    assert np.array_equal(xyz, xyz0[keep]) and np.array_equal(cnt, cnt0[keep])
    # the same crop again removes nothing: NDT_OK, capacity and content as they are
    assert ndt.mapCrop(*base["box"], remove_inside=bool(remove_inside)) == 0
    assert ndt.mapInfo() == info and states_equal(ndt.mapExportState(), filter_state(before, keep))


def test_crop_that_removes_nothing_and_crop_that_removes_everything(pkg, base):
    leaf = 1.0
    ndt = build(pkg, leaf, base["scans"], base["poses"], 64)
    before, info0 = ndt.mapExportState(), ndt.mapInfo()
    assert info0["n_grows"] >= 1
    assert ndt.mapCrop([-1e6] * 3, [1e6] * 3) == 0                                             # everything is inside
    assert ndt.mapCrop([5000.0, 5000.0, 0.0], [5010.0, 5010.0, 10.0], remove_inside=True) == 0  # nothing is inside
    assert ndt.mapCrop([1.0, 1.0, 1.0], [2.0, 0.0, 2.0], remove_inside=True) == 0              # an empty box holds nothing
    assert ndt.mapInfo() == info0 and states_equal(ndt.mapExportState(), before)
    # keep-inside with an empty box empties the map, which still exists and still keeps moments
    assert ndt.mapCrop([1.0, 1.0, 1.0], [2.0, 0.0, 2.0]) == info0["n_voxels"]
    info = ndt.mapInfo()
    assert info["n_voxels"] == 0 and info["n_points"] == 0 and info["capacity"] == 64 and ndt.mapHasMoments()
    assert info["n_adds"] == info0["n_adds"] and info["n_grows"] == info0["n_grows"]
    empty = ndt.mapExportState()
    assert len(empty["count"]) == 0 and empty["moments"].shape == (0, 9) and len(ndt.mapExport()) == 0
    assert ndt.mapCrop(*base["box"]) == 0
    # added to again it equals a fresh map with the same adds
    for s, T in zip(base["scans"], base["poses"]):
        ndt.mapAdd(s, pose=T)
    assert states_equal(ndt.mapExportState(), base["whole"][leaf])
    again = ndt.mapInfo()
    assert again["n_voxels"] == info0["n_voxels"] and again["n_points"] == info0["n_points"]
    assert again["min_ijk"] == info0["min_ijk"] and again["max_ijk"] == info0["max_ijk"]


# ---- 3. crop, then continue ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remove_inside", [0, 1])
@pytest.mark.parametrize("leaf", LEAVES)
def test_crop_then_continue(pkg, base, leaf, remove_inside):
    ndt = build(pkg, leaf, base["moved"][:2], capacity=64)
    first = base["first"][leaf]
    inside = box_mask(first["ijk"], leaf, *base["box"])
    keep = ~inside if remove_inside else inside
    assert ndt.mapCrop(*base["box"], remove_inside=bool(remove_inside)) == int((~keep).sum()) > 0
    for m in base["moved"][2:]:
        ndt.mapAdd(m)
    # survivors continue their sums in input order; dropped voxels seen again restart from the later scans alone
    want = continue_numpy(filter_state(first, keep), np.concatenate(base["moved"][2:]), leaf)
    got = ndt.mapExportState()
    assert states_equal(got, want)
    later = base["second"][leaf]
    dropped_seen_again = np.isin(state_key(later["ijk"]), state_key(first["ijk"][~keep]))
    survived_and_seen = np.isin(state_key(later["ijk"]), state_key(first["ijk"][keep]))
    assert dropped_seen_again.sum() > 20 and survived_and_seen.sum() > 20
    at = np.isin(state_key(got["ijk"]), state_key(later["ijk"][dropped_seen_again]))
    assert states_equal(filter_state(got, at), filter_state(later, dropped_seen_again))
    info = ndt.mapInfo()
    assert info["n_voxels"] == len(want["count"]) and info["n_points"] == int(want["count"].sum())
    assert info["min_ijk"] == tuple(want["ijk"].min(0)) and info["max_ijk"] == tuple(want["ijk"].max(0))


# ---- 3b. growth, crop, carve and growth again: one handle through every replacement of its table ------------------------
def test_every_table_replacement_in_a_row_on_one_handle(pkg):
    """The three replacements share one host tail (map_replace_table) and one device move (map_move_slot).  One map with
    moments and intensity, reset at the smallest capacity (64 slots), takes the carve scene's first two scans (2 x 2 048
    points, a few hundred voxels; both adds grow the table), then a crop that removes the inside of a box, a carve by the
    third scan and a third add that grows the shrunken table again.  After every step the exported state is the
    restatements applied in the same order, bit for bit, and mapInfo's counters and ijk box are the restatement's."""
    leaf = SCENE_LEAF
    scene = carve_scene(cols=64, rows=32)
    rng = np.random.default_rng(11)
    clouds = [np.concatenate([s, rng.uniform(0, 255, (len(s), 1)).astype(np.float32)], axis=1) for s in scene["scans"]]
    assert sum(len(c) for c in clouds[:2]) == 4096
    ndt = engine(pkg, leaf)
    ndt.mapReset(leaf, with_intensity=True, initial_capacity=1)
    ndt.mapEnableMoments()
    assert ndt.mapInfo()["capacity"] == 64

    def check(want, n_grows, capacity):
        assert states_equal(ndt.mapExportState(), want)
        info = ndt.mapInfo()
        assert info["n_voxels"] == len(want["count"]) and info["n_points"] == int(want["count"].sum())
        assert info["min_ijk"] == tuple(want["ijk"].min(0)) and info["max_ijk"] == tuple(want["ijk"].max(0))
        assert info["n_grows"] == n_grows and info["capacity"] == capacity

    ndt.mapAdd(clouds[0], intensity_column=3)
    st = mapstate_numpy(clouds[0][:, :3], leaf, clouds[0][:, 3])
    check(st, 1, 4096)                                                                         # the first add grew the table
    v0 = len(st["count"])
    ndt.mapAdd(clouds[1], intensity_column=3)
    st = continue_numpy(st, clouds[1][:, :3], leaf, clouds[1][:, 3])
    assert 200 <= len(st["count"]) <= 999 and st["sums"][:, 3].any()
    check(st, 2, pow2_at_least(2 * (v0 + 2048)))
    # 1. crop: the inside of a box that holds a piece of the wall and of the ground in front of it goes
    box = ([10.0, 1.0, -2.0], [13.0, 9.0, 4.0])
    inside = box_mask(st["ijk"], leaf, *box)
    assert 20 <= inside.sum() < len(inside) - 100
    assert ndt.mapCrop(*box, remove_inside=True) == int(inside.sum())
    st = filter_state(st, ~inside)
    check(st, 2, pow2_at_least(2 * len(st["count"])))
    # 2. carve: the third scan looks through where the car was
    want = carve_numpy(st["ijk"], st["count"], scene["scans"][2], scene["origin"], leaf, **DEFAULTS)
    assert 1 <= want["n_removed"] < len(st["count"]) - 100
    assert ndt.mapCarve(scene["scans"][2], scene["origin"]) == result_of(want)
    st = filter_state(st, want["keep"])
    check(st, 2, pow2_at_least(2 * len(st["count"])))
    # 3. an add that grows the shrunken table: survivors go on, removed voxels seen again start from this scan alone
    kept = len(st["count"])
    assert pow2_at_least(2 * (kept + 2048)) > pow2_at_least(2 * kept)
    ndt.mapAdd(clouds[2], intensity_column=3)
    st = continue_numpy(st, clouds[2][:, :3], leaf, clouds[2][:, 3])
    check(st, 3, pow2_at_least(2 * (kept + 2048)))


# ---- 4. save, load, continue = never stopped ---------------------------------------------------------------------------
def download(hipmem, ptr, like):
    out = np.zeros_like(like)
    assert hipmem.rt.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0
    return out


@pytest.mark.parametrize("via", ["host", "device"])
@pytest.mark.parametrize("leaf", LEAVES)
def test_save_load_continue_equals_never_stopped(pkg, O, base, hipmem, leaf, via):
    a = build(pkg, leaf, base["scans"][:2], base["poses"][:2])
    b = engine(pkg, leaf)
    b.mapReset(leaf)
    b.mapEnableMoments()
    n = a.mapInfo()["n_voxels"]
    if via == "host":
        st = a.mapExportState()
        assert states_equal(st, base["first"][leaf])
        b.mapImportState(st)
    else:                                                   # between the two handles without a host copy
        d_ijk, d_cnt = hipmem.upload(np.zeros((n, 3), np.int32)), hipmem.upload(np.zeros(n, np.int32))
        d_sums, d_mom = hipmem.upload(np.zeros((n, 4), np.float32)), hipmem.upload(np.zeros((n, 9), np.float64))
        assert a.mapExportStateDevice(d_ijk, d_cnt, d_sums, d_mom, n) == n
        first = base["first"][leaf]
        assert np.array_equal(download(hipmem, d_ijk, first["ijk"]), first["ijk"])
        assert np.array_equal(download(hipmem, d_mom, first["moments"]).view(np.uint64), first["moments"].view(np.uint64))
        b.mapImportStateDevice(leaf, d_ijk, d_cnt, d_sums, d_mom, n)
    ia, ib = a.mapInfo(), b.mapInfo()
    assert ib["n_adds"] == 1 and all(ia[k] == ib[k] for k in ("n_voxels", "n_points", "min_ijk", "max_ijk"))
    for s, T in zip(base["scans"][2:], base["poses"][2:]):
        a.mapAdd(s, pose=T)
        b.mapAdd(s, pose=T)
    sa, sb = a.mapExportState(), b.mapExportState()
    assert states_equal(sa, base["whole"][leaf]) and states_equal(sb, sa)
    xa, xb = export_bits(a), export_bits(b)
    assert np.array_equal(xa[0], xb[0]) and np.array_equal(xa[1], xb[1])
    ia, ib = a.mapInfo(), b.mapInfo()
    assert all(ia[k] == ib[k] for k in ("n_voxels", "n_points", "min_ijk", "max_ijk")) and ib["n_points_dropped"] == 0
    # the targets made from the two maps: the same bytes, and the same 32 words from one evaluation
    p = O.matrix_to_pose(base["poses"][3]) + [0.05, -0.03, 0.02, 0.01, -0.005, 0.008]
    out = []
    for ndt in (a, b):
        ndt.setInputTargetFromMapMoments(*base["box"])
        ndt.setInputSource(base["scans"][3])
        out.append((leaf_bytes(pkg, ndt), eval_words(pkg, ndt, p)))
    assert out[0][0] == out[1][0] and len(out[0][0]) > 0
    assert np.array_equal(out[0][1], out[1][1])


# ---- 5. merge -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", LEAVES)
def test_merge_two_maps(pkg, base, leaf):
    a = build(pkg, leaf, base["moved"][:2])
    b = build(pkg, leaf, base["moved"][2:])
    sa, sb = a.mapExportState(), b.mapExportState()
    assert states_equal(sa, base["first"][leaf]) and states_equal(sb, base["second"][leaf])
    adds = a.mapInfo()["n_adds"]
    a.mapImportState(sb)
    got, whole = a.mapExportState(), base["whole"][leaf]
    assert np.array_equal(got["ijk"], whole["ijk"]) and np.array_equal(got["count"], whole["count"])   # the map of all four
    assert states_equal(got, merge_numpy(sa, sb))
    ka, kb, kg = state_key(sa["ijk"]), state_key(sb["ijk"]), state_key(got["ijk"])
    only_a, only_b = ~np.isin(kg, kb), ~np.isin(kg, ka)
    assert only_a.sum() > 100 and only_b.sum() > 100 and (~only_a & ~only_b).sum() > 100
    assert states_equal(filter_state(got, only_a), filter_state(sa, ~np.isin(ka, kb)))        # one side's records, bit for bit
    assert states_equal(filter_state(got, only_b), filter_state(sb, ~np.isin(kb, ka)))
    info = a.mapInfo()
    assert info["n_adds"] == adds + 1 and info["n_points"] == len(base["cat"]) and info["n_voxels"] == len(whole["count"])
    assert info["min_ijk"] == tuple(whole["ijk"].min(0)) and info["max_ijk"] == tuple(whole["ijk"].max(0))
    assert states_equal(b.mapExportState(), sb)                                                # the source map is as it was


def test_import_with_repeated_voxels_is_applied_in_input_order(pkg, base):
    leaf = 1.0
    sa, sb = base["first"][leaf], base["second"][leaf]
    rng = np.random.default_rng(21)
    pick = np.concatenate([rng.permutation(1200), rng.permutation(1200)[:700], rng.permutation(1200)[:300]])   # up to 3 x
    rec = filter_state(sb, pick)
    a = build(pkg, leaf, base["moved"][:2])
    a.mapImportState(leaf=leaf, ijk=rec["ijk"], count=rec["count"], sums=rec["sums"], moments=rec["moments"])
    # NumPy's sequential restatement: one record at a time, old + record per field
    slot = {int(k): r for r, k in enumerate(state_key(sa["ijk"]))}
    ijk, cnt = [v for v in sa["ijk"]], [int(c) for c in sa["count"]]
    sums, mom = [v.copy() for v in sa["sums"]], [v.copy() for v in sa["moments"]]
    for r, k in enumerate(state_key(rec["ijk"])):
        at = slot.get(int(k))
        if at is None:
            at = slot[int(k)] = len(cnt)
            ijk.append(rec["ijk"][r]); cnt.append(0); sums.append(np.zeros(4, np.float32)); mom.append(np.zeros(9))
        sums[at] = sums[at] + rec["sums"][r]
        mom[at] = mom[at] + rec["moments"][r]
        cnt[at] += int(rec["count"][r])
    order = np.argsort(state_key(np.array(ijk)))
    want = dict(ijk=np.array(ijk, np.int32)[order], count=np.array(cnt, np.int32)[order],
                sums=np.array(sums, np.float32)[order], moments=np.array(mom)[order])
    assert states_equal(a.mapExportState(), want)
    assert a.mapInfo()["n_points"] == int(sa["count"].sum()) + int(rec["count"].sum())


def test_import_grows_a_small_table(pkg, base):
    leaf = 0.5
    sa, sb = base["first"][leaf], base["second"][leaf]
    ndt = engine(pkg, leaf)
    ndt.mapReset(leaf, initial_capacity=64)
    ndt.mapEnableMoments()
    ndt.mapImportState(dict(leaf=leaf, **sa))
    info = ndt.mapInfo()
    assert info["n_grows"] == 1 and info["capacity"] == pow2_at_least(2 * len(sa["count"])) and info["n_voxels"] == len(sa["count"])
    assert states_equal(ndt.mapExportState(), sa)                                              # into an empty map: bit for bit
    ndt.mapImportState(dict(leaf=leaf, **sb))
    assert ndt.mapInfo()["n_grows"] == 2
    assert states_equal(ndt.mapExportState(), merge_numpy(sa, sb))


def test_two_patches_30_km_apart(pkg, base):
    leaf = 0.5
    far = np.float64([21213.25, 21213.25, 0.0])                                   # 30 km along the diagonal
    pa = base["moved"][0]
    pb = (base["moved"][1].astype(np.float64) + far).astype(np.float32)
    both = mapstate_numpy(np.concatenate([pa, pb]), leaf)
    ext = both["ijk"].astype(np.int64)
    assert np.prod((ext.max(0) - ext.min(0) + 1).astype(np.float64)) >= 2**31 - 1   # beyond a dense index: a two-word sort key
    a, b = build(pkg, leaf, [pa]), build(pkg, leaf, [pb])
    a.mapImportState(b.mapExportState())
    assert states_equal(a.mapExportState(), both)                                 # (no voxel is shared: every record as it was)
    margin = np.float32([1.0, 1.0, 1.0])
    in_b = box_mask(both["ijk"], leaf, pb.min(0) - margin, pb.max(0) + margin)
    assert states_equal(a.mapExportState(pb.min(0) - margin, pb.max(0) + margin), filter_state(both, in_b))
    assert a.mapCrop(pb.min(0) - margin, pb.max(0) + margin, remove_inside=True) == int(in_b.sum())
    assert states_equal(a.mapExportState(), mapstate_numpy(pa, leaf))
    info = a.mapInfo()
    assert info["max_ijk"] == tuple(both["ijk"][~in_b].max(0)) and info["min_ijk"] == tuple(both["ijk"][~in_b].min(0))


# ---- 6. refusals leave the map as it was --------------------------------------------------------------------------------
def test_refusals_leave_the_map_as_it_was(pkg, base):
    leaf = 1.0
    L = pkg.lib()
    ndt = engine(pkg, leaf)
    rec = filter_state(base["second"][leaf], slice(0, 200))
    lo, hi = (np.ascontiguousarray(v, np.float32) for v in base["box"])
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    removed, m = C.c_int64(-3), C.c_size_t(77)
    # no map
    assert code_of(pkg, ndt.mapCrop, lo, hi) == INVALID_ARG
    assert code_of(pkg, ndt.mapImportState, dict(leaf=leaf, **rec)) == INVALID_ARG
    assert L.ndt_map_export_state(ndt._h, None, None, None, None, None, None, 0, C.byref(m)) == INVALID_ARG
    assert "no map" in L.ndt_last_error(ndt._h).decode()
    ndt.mapReset(leaf)
    ndt.mapEnableMoments()
    for piece in base["moved"][:2]:
        ndt.mapAdd(piece)
    before, info = ndt.mapExportState(), ndt.mapInfo()

    def unchanged():
        assert ndt.mapInfo() == info and states_equal(ndt.mapExportState(), before)

    def refused(code, **change):
        r = dict(leaf=leaf, ijk=rec["ijk"].copy(), count=rec["count"].copy(), sums=rec["sums"], moments=rec["moments"])
        r.update(change)
        with pytest.raises(pkg.NdtError) as ei:
            ndt.mapImportState(**r)
        assert ei.value.code == code
        unchanged()
        return str(ei.value)

    refused(INVALID_ARG, leaf=0.5)                                                # another leaf size
    refused(INVALID_ARG, leaf=float(np.nextafter(np.float32(leaf), np.float32(2))))   # ... by one bit
    count = rec["count"].copy()
    count[17], count[150] = 0, -4
    assert "2 record(s)" in refused(INVALID_ARG, count=count)                     # count < 1 somewhere in the batch
    for v in (2**20, -(2**20)):
        ijk = rec["ijk"].copy()
        ijk[99, 1] = v
        refused(GRID_OVERFLOW, ijk=ijk)
    refused(INVALID_ARG, moments=None)                                            # a map with moments, a state without
    # boxes, at the C boundary (the Python mirror refuses them before the library: tests/test_map_state_cpu.py)
    nan_box = np.float32([0.0, np.nan, 0.0])
    inf_box = np.float32([np.inf, 0.0, 0.0])
    assert L.ndt_map_crop(ndt._h, fp(lo), None, 0, C.byref(removed)) == INVALID_ARG            # half a box
    assert L.ndt_map_crop(ndt._h, None, None, 0, C.byref(removed)) == INVALID_ARG
    assert L.ndt_map_crop(ndt._h, fp(nan_box), fp(hi), 0, C.byref(removed)) == INVALID_ARG     # non-finite
    assert L.ndt_map_crop(ndt._h, fp(lo), fp(inf_box), 1, C.byref(removed)) == INVALID_ARG
    assert L.ndt_map_export_state(ndt._h, fp(lo), None, None, None, None, None, 0, C.byref(m)) == INVALID_ARG
    assert L.ndt_map_export_state(ndt._h, fp(lo), fp(nan_box), None, None, None, None, 0, C.byref(m)) == INVALID_ARG
    assert removed.value == -3 and m.value == 77
    unchanged()
    # n = 0 is a no-op; a voxel at the edge of the coordinate range is taken
    ndt.mapImportState(dict(leaf=leaf, **filter_state(rec, slice(0, 0))))
    unchanged()
    edge = filter_state(rec, slice(0, 2))
    edge["ijk"] = np.int32([[2**20 - 1, 0, 0], [0, -(2**20) + 1, 0]])
    ndt.mapImportState(dict(leaf=leaf, **edge))
    now = ndt.mapInfo()
    assert now["n_voxels"] == info["n_voxels"] + 2 and now["max_ijk"][0] == 2**20 - 1 and now["min_ijk"][1] == -(2**20) + 1
    ndt.mapClear()
    assert code_of(pkg, ndt.mapCrop, lo, hi) == INVALID_ARG                       # after mapClear: no map again


# ---- 7. the rest of the handle is left alone ----------------------------------------------------------------------------
def test_the_rest_of_the_handle_is_left_alone(pkg, O, base):
    leaf = 1.0
    ndt = build(pkg, leaf, base["scans"], base["poses"])
    ndt.setInputTargetFromMapMoments(*base["box"])                                # a target made from this very map
    ndt.setInputSource(base["scans"][3])
    ndt.putKeyframe(7, base["scans"][0])
    ndt.align(base["poses"][3])
    p = O.matrix_to_pose(base["poses"][3]) + [0.05, -0.03, 0.02, 0.01, -0.005, 0.008]
    words = eval_words(pkg, ndt, p)

    def state():
        h = ndt.getIterationHistory()
        return (leaf_bytes(pkg, ndt), ndt.sourceSize(), [a.tobytes() for a in h], ndt.getTiming()["n_eval_launches"],
                ndt.keyframeCount(), ndt.getFinalTransformation().tobytes(), ndt.getGridInfo()["n_target_points"])

    before = state()
    c0 = base["poses"][0][:3, 3]
    region = (c0 - [8.0, 8.0, 4.0], c0 + [8.0, 8.0, 4.0])                         # around the first pose: 173 voxels
    cut = ndt.mapExportState(*region)
    assert len(cut["count"]) > 100
    assert ndt.mapCrop(*region, remove_inside=True) == len(cut["count"])          # erase a region ...
    ndt.mapImportState(cut)                                                       # ... and put it back
    assert states_equal(ndt.mapExportState(), base["whole"][leaf])
    assert ndt.mapCrop(*base["box"]) > 0                                          # the sliding window
    assert state() == before
    assert np.array_equal(eval_words(pkg, ndt, p), words)
    # a target made from the cropped map: the oracle on the points whose voxel survived
    cat = base["cat"]
    sub = cat[in_box(cat, leaf, *base["box"])]
    assert 0 < len(sub) < len(cat)
    grid = O.Grid(sub, oracle_params(O, leaf))
    ndt.setInputTargetFromMapMoments()
    assert_grid_matches(ndt.getGridInfo(), grid, len(sub))
    assert_leaves_match(ndt.getLeaves(), grid.export(), 1e-9, "whole-map target after a crop to the box")


# ---- 8. the C++ adapter -----------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, tmp_path):
    """tests/cpp/test_map_state.cpp against the API mocks, built with the g++ line tests/cpp/Makefile uses for them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "tests", "cpp")
    exe = str(tmp_path / "test_map_state")
    lib = os.path.join(root, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(root, "include", "compat"), "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(d, "test_map_state.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "map state: PASS" in p.stdout
