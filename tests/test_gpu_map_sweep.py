"""The voxel-map family swept at inexact leaf sizes and on voxel faces: one engine per case of
tests/test_map_sweep_cpu.py (`cases()`: leaf 0.1, 0.3, 0.7, 1.5, 1.7 and the exact-inverse control 0.5; four scene centres out
to 29 km; five kinds of cloud scaled by the leaf; ragged pieces; non-finite rows; intensity; a table grown from 64 slots;
moments on / off; a face set in every cloud of 700 points and more), every stage against the restatement the project already
has for it -- none is restated here, and that file pins the restatements to the oracle and to the dense index at these leaves:

  add -> export        voxelmap_numpy (test_gpu_voxel_map)                    bits
  moments              moments_numpy (test_map_target_cpu)                    bits
  state, box export    mapstate_numpy / filter_state + box_mask               bits
  target from moments  the oracle on the concatenation: grid, cells, counts exact; mean 1e-12; covariance by
                       test_gpu_random.cov_loss (per leaf, and its largest value through assert_leaves_match); evaluation
                       against the oracle's f64 formulas (pair_mode = 2) with test_random_cloud_parity's assertions
  Gaussian source      the leaves of that target                              bits
  crop, then add       filter_state, continue_numpy                           bits
  carve                carve_numpy through test_gpu_map_carve.check_carve     every field ==, state bits
  transform, then add  repose_numpy, continue_numpy                           bits
  posed import         repose_numpy(..., into=...)                            bits

Every bound is copied from the test named next to it; no tolerance is new.  Two edge tests follow: the coordinate limit at
leaf 0.3, and box corners one f32 step either side of a face at leaf 0.3 and 0.7."""
import time

import numpy as np
import pytest

from test_gpu_d2d import upper6
from test_gpu_map_carve import check_carve
from test_gpu_map_state import box_mask
from test_gpu_map_target import assert_grid_matches, assert_leaves_match, engine, oracle_params
from test_gpu_random import cov_loss
from test_gpu_voxel_map import assert_equals_b, export_bits
from test_map_repose_cpu import repose_numpy, rigid_pose
from test_map_state_cpu import continue_numpy, filter_state, mapstate_numpy, states_equal
from test_map_sweep_cpu import case_id, cases, face_values, has_target, make_case, pieces_of, source_of
from test_map_target_cpu import host_transform_f64, moments_numpy, voxel_ijk

pytestmark = pytest.mark.gpu

GRID_OVERFLOW = -6


def new_map(pkg, d, pieces, first_only=False):
    """A fresh engine whose map took the case's pieces in order (first_only: the first piece alone), then -- in the cases
    that carry a pose -- the first piece once more under it."""
    case = d["case"]
    icol = 3 if case["intensity"] else None
    ndt = engine(pkg, case["leaf"])
    ndt.mapReset(case["leaf"], with_intensity=case["intensity"], initial_capacity=case["capacity"])
    if case["moments"]:
        ndt.mapEnableMoments()
    for p in pieces[:1] if first_only else pieces:
        ndt.mapAdd(p, intensity_column=icol)
    if d["pose"] is not None and not first_only:
        ndt.mapAdd(pieces[0], intensity_column=icol, pose=d["pose"])
    return ndt


def assert_info(info, st):
    assert info["n_voxels"] == len(st["count"]) and info["n_points"] == int(st["count"].sum())
    assert info["min_ijk"] == tuple(st["ijk"].min(0)) and info["max_ijk"] == tuple(st["ijk"].max(0))


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_map_family_on_faces(pkg, O, S, case):
    clock = [("start", time.perf_counter())]
    d = make_case(case)
    leaf, moments, icol = case["leaf"], case["moments"], 3 if case["intensity"] else None
    pieces = pieces_of(d)
    seen, seen_i = d["seen"], d["seen_intensity"]
    fin = np.isfinite(seen).all(axis=1)
    want = mapstate_numpy(seen, leaf, seen_i)
    last, last_i = pieces[-1][:, :3], (pieces[-1][:, 3] if icol else None)
    clock.append(("restate", time.perf_counter()))

    # ---- 1. add -> export ----
    ndt = new_map(pkg, d, pieces)
    assert_equals_b(ndt, seen, leaf, seen_i)
    info = ndt.mapInfo()
    ijk = voxel_ijk(seen[fin], leaf)
    assert info["n_points"] == int(fin.sum()) and info["n_points_dropped"] == int((~fin).sum())
    assert info["min_ijk"] == tuple(ijk.min(0)) and info["max_ijk"] == tuple(ijk.max(0))
    assert info["leaf"] == np.float32(leaf) and info["with_intensity"] == case["intensity"]
    if case["capacity"]:
        assert info["n_grows"] >= 1
    assert info["capacity"] >= 2 * info["n_voxels"]

    # ---- 2. moments ----
    if moments:
        mijk, mcount, msums = ndt.mapExportMoments()
        bijk, bcount, bsums = moments_numpy(seen, leaf)
        assert np.array_equal(mijk, bijk) and np.array_equal(mcount, bcount)
        assert np.array_equal(msums.view(np.uint64), bsums.view(np.uint64))           # the bits of all nine sums
    clock.append(("add, export, moments", time.perf_counter()))

    # ---- 3. state, and the state of a box whose corners are face points ----
    st = ndt.mapExportState()
    assert (st["moments"] is None) == (not moments)
    assert states_equal(st, want, moments=moments)
    assert_info(info, want)
    inside = box_mask(want["ijk"], leaf, *d["box"])
    assert states_equal(ndt.mapExportState(*d["box"]), filter_state(want, inside), moments=moments)
    clock.append(("state", time.perf_counter()))

    # ---- 4. the target made from the moments; 5. the Gaussian source made from the same state ----
    if has_target(case):
        prm = oracle_params(O, leaf)
        grid = O.Grid(seen, prm)
        OL = grid.export()
        assert grid.n_leaves >= 100
        loss = cov_loss(OL)
        amp = float(loss.max())
        ndt.setInputTargetFromMapMoments()
        assert_grid_matches(ndt.getGridInfo(), grid, int(fin.sum()))
        L = ndt.getLeaves()
        assert_leaves_match(L, OL, amp, "moments target vs oracle [%s]" % case_id(case))
        scale = np.abs(OL["cov"]).max(axis=(1, 2))
        assert ((np.abs(L["cov"] - OL["cov"]).max(axis=(1, 2)) / scale) < loss).all()  # (per leaf, as test_random_cloud_parity)
        ref = engine(pkg, leaf)
        ref.setInputTarget(seen[fin])
        gi, gr = ndt.getGridInfo(), ref.getGridInfo()
        for k in ("min_b", "max_b", "div_b"):
            assert np.array_equal(gi[k], gr[k])
        assert gi["n_cells"] == gr["n_cells"] and gi["n_leaves"] == gr["n_leaves"] and gi["n_target_points"] == gr["n_target_points"]
        assert_leaves_match(L, ref.getLeaves(), amp, "moments target vs setInputTarget [%s]" % case_id(case))
        src, poses = source_of(d, S, O)
        ndt.setInputSource(src)
        pairs = {}
        for method, omethod in ((pkg.DIRECT7, O.DIRECT7), (pkg.DIRECT1, O.DIRECT1)):
            ndt.setParams(search_method=method)
            prm64 = oracle_params(O, leaf, search_method=omethod, pair_mode=2)    # the reference's formulas carried in f64
            for p, e in zip(poses, ndt.evalDerivatives(poses)):
                x = grid.derivatives(src, p, params=prm64)
                assert e["n_pairs"] == x["n_pairs"] and e["n_with_neighbors"] == x["n_with_neighbors"]
                assert e["score"] == pytest.approx(x["score"], rel=1e-8 + amp, abs=1e-9)
                gn, hn = np.linalg.norm(x["gradient"]), np.linalg.norm(x["hessian"])
                assert np.linalg.norm(e["gradient"] - x["gradient"]) <= (1e-9 + 30 * amp) * gn + 1e-9
                assert np.linalg.norm(e["hessian"] - x["hessian"]) <= (1e-9 + 30 * amp) * hn + 1e-9
            pairs[method] = ndt.evalDerivatives(poses[0])[0]["n_pairs"]
        print("target [%s]: %d leaves, cov_loss up to %.2e, %d / %d pairs under DIRECT7 / DIRECT1 at the near pose"
              % (case_id(case), grid.n_leaves, amp, pairs[pkg.DIRECT7], pairs[pkg.DIRECT1]))
        assert pairs[pkg.DIRECT7] >= 500
        ndt.setParams(search_method=pkg.DIRECT7)
        clock.append(("target", time.perf_counter()))
        n_rec, n_acc = pkg.setSourceDistributions(ndt, st)
        G = pkg.getSourceDistributions(ndt)
        assert n_rec == len(st["count"]) and n_acc == len(L["count"])
        assert np.array_equal(G["count"], L["count"])
        assert np.array_equal(G["mean"].view(np.uint64), L["mean"].view(np.uint64))                  # bit for bit
        assert np.array_equal(G["cov6"].view(np.uint64), upper6(L["cov"]).view(np.uint64))
        assert np.all(np.diff(G["record_index"]) > 0)                                                # input order
        assert np.array_equal(st["count"][G["record_index"]], G["count"])
        clock.append(("gaussian source", time.perf_counter()))

    # ---- 6. crop to a face-point box, then go on with the last piece ----
    in_crop = box_mask(want["ijk"], leaf, *d["crop"])
    keep = ~in_crop if case["remove_inside"] else in_crop
    assert ndt.mapCrop(*d["crop"], remove_inside=bool(case["remove_inside"])) == int((~keep).sum())
    kept = filter_state(want, keep)
    assert states_equal(ndt.mapExportState(), kept, moments=moments)
    assert_info(ndt.mapInfo(), kept)
    ndt.mapAdd(pieces[-1], intensity_column=icol)
    again = continue_numpy(kept, last, leaf, last_i)
    assert states_equal(ndt.mapExportState(), again, moments=moments)
    assert_info(ndt.mapInfo(), again)
    clock.append(("crop", time.perf_counter()))

    # ---- 7. carve, on a fresh map of the same cloud ----
    carved = new_map(pkg, d, pieces)
    before, res = check_carve(carved, d["rays"], d["carve_origin"], d["carve_pose"], 64 if case["capacity"] else 1 << 18,
                              moments=moments, leaf=leaf, **case["carve_params"])
    assert states_equal(before, want, moments=moments)
    assert 1 <= res["n_removed"] < len(want["count"])
    clock.append(("carve", time.perf_counter()))

    # ---- 8. transform, on a fresh map, then one add on top ----
    T = rigid_pose(t=np.array([10.3, -4.7, 0.21]) * leaf)
    moved = new_map(pkg, d, pieces)
    want_t = repose_numpy(want, T, leaf)
    assert pkg.mapTransform(moved, T) == len(want_t["count"])
    got = moved.mapExportState()
    assert (got["moments"] is None) == (not moments) and moved.mapHasMoments() == moments
    assert states_equal(got, want_t, moments=moments)
    assert_info(moved.mapInfo(), want_t)
    with np.errstate(invalid="ignore"):
        more = host_transform_f64(T, last)
    moved.mapAdd(more if icol is None else np.concatenate([more, last_i[:, None]], axis=1), intensity_column=icol)
    on_top = continue_numpy(want_t, more, leaf, last_i)
    assert states_equal(moved.mapExportState(), on_top, moments=moments)
    assert_info(moved.mapInfo(), on_top)
    clock.append(("transform", time.perf_counter()))

    # ---- 9. the whole state imported under the pose into a second map that holds the first piece ----
    second = new_map(pkg, d, pieces, first_only=True)
    held = mapstate_numpy(pieces[0][:, :3], leaf, pieces[0][:, 3] if icol else None)
    assert states_equal(second.mapExportState(), held, moments=moments)
    rec = dict(leaf=leaf, ijk=want["ijk"], count=want["count"], sums=want["sums"], moments=want["moments"] if moments else None)
    pkg.mapImportStatePosed(second, rec, T)
    merged = repose_numpy(want, T, leaf, into=held)
    assert states_equal(second.mapExportState(), merged, moments=moments)
    assert_info(second.mapInfo(), merged)
    clock.append(("posed import", time.perf_counter()))
    print("stages [%s]: %s; total %.2f s" % (case_id(case), ", ".join("%s %.2f" % (n, t - clock[k][1]) for k, (n, t) in enumerate(clock[1:])),
                                            clock[-1][1] - clock[0][1]))


# ---- the coordinate limit at an inexact leaf ------------------------------------------------------------------------------
def limit_pair(leaf, k):
    """(the largest f32 x with floor(x * inv_leaf) < k, the smallest with floor(x * inv_leaf) >= k), k > 0, in the map's f32
    arithmetic"""
    inv = np.float32(1.0) / np.float32(leaf)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    x = np.float32(k * leaf)
    while np.floor(x * inv) >= k:
        x = np.nextafter(x, down)
    while np.floor(np.nextafter(x, up) * inv) < k:
        x = np.nextafter(x, up)
    return x, np.nextafter(x, up)


def mirror_pair(leaf, k):
    """(the smallest f32 x with floor(x * inv_leaf) > -k, the largest with floor(x * inv_leaf) <= -k)"""
    inv = np.float32(1.0) / np.float32(leaf)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    x = np.float32(-k * leaf)
    while np.floor(x * inv) <= -k:
        x = np.nextafter(x, up)
    while np.floor(np.nextafter(x, down) * inv) > -k:
        x = np.nextafter(x, down)
    return x, np.nextafter(x, down)


def test_the_coordinate_limit_at_an_inexact_leaf(pkg):
    """What test_one_crowded_voxel_and_the_edges_of_the_index and test_refusals_leave_the_map_as_it_was do at 0.5, at 0.3:
    the last accepted x is the largest f32 whose f32 product floors to 2^20 - 1, and the next f32 is refused."""
    leaf, k = 0.3, 2**20
    inv = np.float32(1.0) / np.float32(leaf)
    top_in, top_out = limit_pair(leaf, k)
    low_in, low_out = mirror_pair(leaf, k)
    assert np.floor(top_in * inv) == k - 1 and np.floor(top_out * inv) == k
    assert np.floor(low_in * inv) == -k + 1 and np.floor(low_out * inv) == -k
    # the quotient names another voxel for at least one of the four: the limit is the product's
    four = np.float32([top_in, top_out, low_in, low_out]).astype(np.float64) / np.float64(np.float32(leaf))
    print("limit at leaf 0.3: x = %r | %r and %r | %r, quotients %s" % (top_in, top_out, low_in, low_out, four.tolist()))
    ndt = engine(pkg, leaf)
    ndt.mapReset(leaf)
    inside = np.float32([[top_in, 0.1, 0.1], [low_in, 0.1, -0.1], [0.1, top_in, low_in]])
    ndt.mapAdd(inside)
    info = ndt.mapInfo()
    assert info["max_ijk"][0] == k - 1 and info["min_ijk"][0] == -k + 1
    assert info["max_ijk"][1] == k - 1 and info["min_ijk"][2] == -k + 1 and info["n_points"] == 3
    assert_equals_b(ndt, inside, leaf)
    kept, kept_cnt = export_bits(ndt)
    for a, x in ((0, top_out), (0, low_out), (1, top_out), (2, low_out)):
        far = np.float32([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2]])
        far[1, a] = x
        with pytest.raises(pkg.NdtError) as ei:
            ndt.mapAdd(far)
        assert ei.value.code == GRID_OVERFLOW
        now, now_cnt = export_bits(ndt)
        assert np.array_equal(now, kept) and np.array_equal(now_cnt, kept_cnt) and ndt.mapInfo() == info
    assert_equals_b(ndt, inside, leaf)


# ---- box corners one f32 step either side of a face ------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [0.3, 0.7])
def test_box_corners_one_step_either_side_of_a_face(pkg, leaf):
    """A crop's or a box export's corner on a voxel face, one f32 step below it and one above: the voxel on the face belongs
    to the box exactly when box_mask -- the add's own f32 floor on the corner -- says so, as box_min and as box_max."""
    rng = np.random.default_rng(int(leaf * 10))
    ks = 100 + np.arange(-9, 10)                             # (around voxel 100: 8 and more of these 57 corner values differ)
    pts = ((rng.uniform(-1, 1, (2500, 3)) * [12.0, 3.0, 2.0] + [100.0, 0.0, 0.0]) * leaf).astype(np.float32)
    on_faces = np.zeros((3 * len(ks), 3), np.float32)
    on_faces[:, 0] = face_values(ks, leaf)                                       # points on the very faces the corners name
    on_faces[:, 1:] = (rng.uniform(-1, 1, (len(on_faces), 2)) * leaf).astype(np.float32)
    cloud = np.concatenate([pts, on_faces])[rng.permutation(len(pts) + len(on_faces))]
    want = mapstate_numpy(cloud, leaf)

    def fresh():
        m = engine(pkg, leaf)
        m.mapReset(leaf, initial_capacity=64)
        m.mapEnableMoments()
        m.mapAdd(cloud)
        return m

    ndt = fresh()
    assert states_equal(ndt.mapExportState(), want)
    big = np.float32(1000.0 * leaf)
    differs, flips = 0, 0
    for k in ks:
        members = ([], [])
        for v in face_values([k], leaf):
            q = int(np.floor(np.float64(v) / np.float64(np.float32(leaf))))
            differs += q != int(voxel_ijk(np.float32([[v, 0, 0]]), leaf)[0, 0])
            # as box_min the face decides about the voxels k - 1, as box_max about the voxels k
            for which, (lo, hi) in enumerate((([v, -big, -big], [big, big, big]), ([-big, -big, -big], [v, big, big]))):
                inside = box_mask(want["ijk"], leaf, lo, hi)
                assert 0 < inside.sum() < len(inside)
                assert states_equal(ndt.mapExportState(lo, hi), filter_state(want, inside))
                row = inside[want["ijk"][:, 0] == k - 1 + which]
                assert len(row) and row.all() == row.any()                       # the voxels beside the face go as one
                members[which].append(bool(row.all()))
        flips += (len(set(members[0])) > 1) + (len(set(members[1])) > 1)
    print("leaf %g: %d of %d corner values floor differently under the quotient; the voxels beside a face change sides within one "
          "f32 step of it in %d of %d face / corner pairs" % (leaf, differs, 3 * len(ks), flips, 2 * len(ks)))
    assert differs >= 8 and flips >= 2
    # the crop itself, at the faces where the quotient would have decided otherwise (and at two more)
    odd = [k for k in ks if any(int(np.floor(np.float64(v) / np.float64(np.float32(leaf)))) != int(voxel_ijk(np.float32([[v, 0, 0]]), leaf)[0, 0])
                                for v in face_values([k], leaf))]
    for k in (odd[:2] + [int(ks[0]), int(ks[-1])]):
        for v in face_values([k], leaf):
            for remove_inside, (lo, hi) in ((0, ([v, -big, -big], [big, big, big])), (1, ([-big, -big, -big], [v, big, big]))):
                m = fresh()
                inside = box_mask(want["ijk"], leaf, lo, hi)
                keep = ~inside if remove_inside else inside
                assert m.mapCrop(lo, hi, remove_inside=bool(remove_inside)) == int((~keep).sum())
                assert states_equal(m.mapExportState(), filter_state(want, keep))
