"""The voxel map under a changed pose (ndt_map_transform, ndt_map_import_state_posed / _device) against the NumPy
restatement of the header's rule (test_map_repose_cpu.repose_records / merge_records / repose_numpy), bit for bit, and on
lattice scenes against a second map fed the moved points.
Scenes: `small` about 300 occupied voxels (two blocks of records with a ragged tail), `large` about 5 000; both scale with
the leaf, hold negative coordinates, a few non-finite points and up to a few dozen points per voxel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_map_target import code_of, engine, eval_words, leaf_bytes
from test_map_repose_cpu import (LATTICE_POSES, affine, lattice_scene, merge_records, move_points, repose_numpy, repose_records,
                                 rigid_pose)
from test_map_state_cpu import continue_numpy, filter_state, mapstate_numpy, state_key, states_equal
from test_map_target_cpu import host_transform_f64, voxel_ijk

pytestmark = pytest.mark.gpu

INVALID_ARG, GRID_OVERFLOW = -1, -6
RIGID = rigid_pose()


def pow2_at_least(v):
    c = 64
    while c < v:
        c <<= 1
    return c


def scene(size, leaf, seed=0):
    """(points [n, 3] float32 with 7 non-finite rows, intensity [n] float32): uniform over a box of 10 x 8 x 4 (small) or
    30 x 24 x 7 (large) voxels, five points per voxel on average"""
    dims = np.array({"small": (10, 8, 4), "large": (30, 24, 7)}[size], np.float64)
    rng = np.random.default_rng(seed + (1 if size == "large" else 0))
    n = int(5 * dims.prod())
    pts = ((rng.uniform(0, 1, (n, 3)) * dims - dims * [0.5, 0.25, 0.5]) * leaf).astype(np.float32)
    pts[::max(n // 7, 1)][:7] = np.nan
    pts[3::max(n // 7, 1)][:7] = np.nan
    return pts, rng.uniform(0, 255, n).astype(np.float32)


def build(pkg, leaf, pieces, moments=True, intensity=False, capacity=64, **kw):
    ndt = engine(pkg, leaf, **kw)
    ndt.mapReset(leaf, with_intensity=intensity, initial_capacity=capacity)
    if moments:
        ndt.mapEnableMoments()
    for p in pieces:
        ndt.mapAdd(p, intensity_column=3 if intensity else None)
    return ndt


def strip(st, moments):
    return st if moments else dict(st, moments=None)


def counters(info):
    return {k: info[k] for k in ("n_points", "n_points_dropped", "n_adds", "n_grows")}


def assert_info_after_transform(info, before, want, reset_capacity):
    assert counters(info) == counters(before)
    assert info["n_voxels"] == len(want["count"]) <= before["n_voxels"]
    assert info["min_ijk"] == tuple(want["ijk"].min(0)) and info["max_ijk"] == tuple(want["ijk"].max(0))      # the tight box
    assert info["capacity"] == max(pow2_at_least(2 * before["n_voxels"]), reset_capacity)
    assert info["leaf"] == before["leaf"] and info["with_intensity"] == before["with_intensity"]


# ---- 1. the transform is the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("size,leaf", [("small", 1.0), ("small", 0.5), ("large", 1.0), ("large", 0.5)])
@pytest.mark.parametrize("moments", [True, False], ids=["moments", "nomoments"])
@pytest.mark.parametrize("intensity", [True, False], ids=["intensity", "xyz"])
def test_transform_equals_the_restatement(pkg, size, leaf, moments, intensity):
    pts, inten = scene(size, leaf)
    cloud = np.concatenate([pts, inten[:, None]], axis=1) if intensity else pts
    ndt = build(pkg, leaf, np.array_split(cloud, 3), moments, intensity)
    st = strip(mapstate_numpy(pts, leaf, inten if intensity else None), moments)
    n = len(st["count"])
    assert (257 <= n <= 511) if size == "small" else (4000 <= n <= 6000)
    assert states_equal(ndt.mapExportState(), st, moments=moments)
    before = ndt.mapInfo()
    assert before["n_points_dropped"] > 0 and before["n_grows"] > 0
    want = repose_numpy(st, RIGID, leaf)
    assert len(want["count"]) < n                                                   # a general pose merges some voxels
    assert pkg.mapTransform(ndt, RIGID) == len(want["count"])
    got = ndt.mapExportState()
    assert (got["moments"] is None) == (not moments) and ndt.mapHasMoments() == moments
    assert states_equal(got, want, moments=moments)
    assert_info_after_transform(ndt.mapInfo(), before, want, 64)
    if intensity:
        assert want["sums"][:, 3].any()
    # ... and back: the inverse pose is one more application of the rule, not an undo
    back = repose_numpy(want, np.linalg.inv(RIGID), leaf)
    pkg.mapTransform(ndt, np.linalg.inv(RIGID))
    assert states_equal(ndt.mapExportState(), back, moments=moments)


# ---- 2. lattice symmetries: the moved map is the map of the moved points ------------------------------------------------
@pytest.fixture(scope="module")
def lattice():
    pts = lattice_scene()
    return pts, mapstate_numpy(pts, 0.5)


@pytest.mark.parametrize("name", ["shift", "rz90", "flip", "cycle"])
def test_lattice_symmetries(pkg, lattice, name):
    pts, st = lattice
    T = LATTICE_POSES[name]
    a = build(pkg, 0.5, np.array_split(pts, 2))
    b = build(pkg, 0.5, np.array_split(move_points(T, pts), 2))
    assert pkg.mapTransform(a, T) == 300
    got, direct = a.mapExportState(), b.mapExportState()
    assert states_equal(got, direct)
    assert states_equal(got, repose_numpy(st, T, 0.5))
    assert a.mapInfo()["min_ijk"] == b.mapInfo()["min_ijk"] and a.mapInfo()["max_ijk"] == b.mapInfo()["max_ijk"]
    assert np.array_equal(a.mapExport().view(np.uint32), b.mapExport().view(np.uint32))       # the centroids as bits


# ---- 3. many voxels into one: runs are applied in input order ----------------------------------------------------------
def test_many_into_one(pkg):
    leaf = 0.5
    pts, _ = scene("large", leaf, seed=2)
    T = affine(np.diag([0.25, 0.25, 0.25]), (1.0, -1.5, 0.5))                    # the 3 x 4 as given: no rigidity check
    ndt = build(pkg, leaf, [pts])
    st = mapstate_numpy(pts, leaf)
    rec, bad = repose_records(st, T, leaf)
    assert bad == 0
    _, runs = np.unique(state_key(rec["ijk"]), return_counts=True)
    assert 32 <= runs.max() <= 64 and len(runs) < len(st["count"]) // 20
    want = merge_records(None, rec)
    # the order matters in this scene: merging the same records in descending order gives other bits
    rev = {k: v[::-1] for k, v in rec.items()}
    assert not states_equal(merge_records(None, rev), want)
    before = ndt.mapInfo()
    assert pkg.mapTransform(ndt, T) == len(want["count"])
    assert states_equal(ndt.mapExportState(), want)
    assert_info_after_transform(ndt.mapInfo(), before, want, 64)


# ---- 4. posed import -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_posed_import(pkg, hipmem, form):
    leaf = 1.0
    pts, _ = scene("large", leaf, seed=4)
    pts = pts[np.isfinite(pts).all(axis=1)]
    half = len(pts) // 2
    a_pts = pts[:half]
    b_local = host_transform_f64(np.linalg.inv(RIGID), pts[half:])                  # the other half in its own frame
    A = mapstate_numpy(a_pts, leaf)
    B = mapstate_numpy(b_local, leaf)
    # records that repeat a destination voxel: a third of B's records once more, shuffled, behind the first pass
    again = np.random.default_rng(9).permutation(len(B["count"]))[:len(B["count"]) // 3]
    recs = {k: np.concatenate([B[k], B[k][again]]) for k in ("ijk", "count", "sums", "moments")}
    want = repose_numpy(recs, RIGID, leaf, into=A)
    ndt = build(pkg, leaf, np.array_split(a_pts, len(a_pts) // 256), capacity=1 << 10)           # small adds: a tight table
    assert states_equal(ndt.mapExportState(), A)
    before = ndt.mapInfo()
    assert before["capacity"] < 2 * (before["n_voxels"] + len(recs["count"]))
    if form == "host":
        pkg.mapImportStatePosed(ndt, dict(recs, leaf=leaf), RIGID)
    else:
        pkg.mapImportStatePosedDevice(ndt, leaf, hipmem.upload(recs["ijk"]), hipmem.upload(recs["count"]), hipmem.upload(recs["sums"]),
                                      hipmem.upload(recs["moments"]), len(recs["count"]), RIGID)
    assert states_equal(ndt.mapExportState(), want)
    info = ndt.mapInfo()
    assert info["n_grows"] > before["n_grows"] and info["n_adds"] == before["n_adds"] + 1
    assert info["n_points"] == before["n_points"] + int(recs["count"].sum()) and info["n_voxels"] == len(want["count"])
    assert info["min_ijk"] == tuple(want["ijk"].min(0)) and info["max_ijk"] == tuple(want["ijk"].max(0))
    # a map without moments ignores them and bins by the same float centroid
    plain = build(pkg, leaf, np.array_split(a_pts, 4), moments=False)
    pkg.mapImportStatePosed(plain, dict(recs, leaf=leaf, moments=None), RIGID)
    assert states_equal(plain.mapExportState(), dict(want, moments=None), moments=False)


# ---- 5. two patches 30 km apart move together ---------------------------------------------------------------------------
def test_two_patches_30_km_apart(pkg):
    leaf = 0.5
    a, _ = scene("small", leaf, seed=5)
    b = (scene("small", leaf, seed=6)[0].astype(np.float64) + [21213.25, 21213.25, 0.0]).astype(np.float32)
    both = np.concatenate([a, b])
    ext = voxel_ijk(both[np.isfinite(both).all(axis=1)], leaf)
    assert np.prod((ext.max(0) - ext.min(0) + 1).astype(np.float64)) >= 2**31 - 1   # no dense index holds this map
    ndt = build(pkg, leaf, [a, b])
    want = repose_numpy(mapstate_numpy(both, leaf), RIGID, leaf)
    before = ndt.mapInfo()
    pkg.mapTransform(ndt, RIGID)
    assert states_equal(ndt.mapExportState(), want)
    assert_info_after_transform(ndt.mapInfo(), before, want, 64)


# ---- 6. identity, empty map ----------------------------------------------------------------------------------------------
def test_identity_and_empty_map(pkg, lattice):
    pts, st = lattice
    ndt = build(pkg, 0.5, [pts])
    assert pkg.mapTransform(ndt, np.eye(4)) == 300
    assert states_equal(ndt.mapExportState(), st)
    empty = build(pkg, 0.5, [])
    before = empty.mapInfo()
    assert pkg.mapTransform(empty, RIGID) == 0
    assert empty.mapInfo() == before and len(empty.mapExportState()["count"]) == 0
    empty.mapAdd(pts)                                                              # ... and it is still a map
    assert states_equal(empty.mapExportState(), st)


# ---- 7. transform, then go on ---------------------------------------------------------------------------------------------
def test_transform_then_continue(pkg):
    leaf = 1.0
    pts, _ = scene("large", leaf, seed=7)
    more, _ = scene("small", leaf, seed=8)
    ndt = build(pkg, leaf, [pts])
    moved = repose_numpy(mapstate_numpy(pts, leaf), RIGID, leaf)
    pkg.mapTransform(ndt, RIGID)
    more = host_transform_f64(RIGID, more)
    ndt.mapAdd(more)
    want = continue_numpy(moved, more, leaf)
    assert states_equal(ndt.mapExportState(), want)
    # crop to the middle half, then export -> import into a fresh handle
    lo, hi = want["ijk"].min(0), want["ijk"].max(0)
    quarter = (hi - lo) // 4
    bmin, bmax = (lo + quarter + 0.5) * leaf, (hi - quarter + 0.5) * leaf
    keep = ((want["ijk"] >= lo + quarter) & (want["ijk"] <= hi - quarter)).all(axis=1)
    assert 0 < keep.sum() < len(keep)
    assert ndt.mapCrop(bmin, bmax) == int((~keep).sum())
    kept = filter_state(want, keep)
    st = ndt.mapExportState()
    assert states_equal(st, kept)
    fresh = build(pkg, leaf, [])
    fresh.mapImportState(st)
    assert states_equal(fresh.mapExportState(), kept)


# ---- 8. refusals leave the map as it was ---------------------------------------------------------------------------------
def test_refusals_leave_the_map_as_it_was(pkg):
    leaf = 0.5
    L = pkg.lib()
    dp = C.POINTER(C.c_double)
    none = engine(pkg, leaf)
    assert code_of(pkg, pkg.mapTransform, none, RIGID) == INVALID_ARG                    # no map
    pts, _ = scene("small", leaf, seed=10)
    ndt = build(pkg, leaf, [pts])
    st, info = ndt.mapExportState(), ndt.mapInfo()
    n = len(st["count"])

    def unchanged():
        return states_equal(ndt.mapExportState(), st) and ndt.mapInfo() == info

    def col(T):
        return np.ascontiguousarray(np.asarray(T, np.float64).T).ravel()

    rec = {k: st[k][:40].copy() for k in ("ijk", "count", "sums", "moments")}
    args = lambda r, mom=True: (ndt._h, C.c_float(leaf), r["ijk"].ctypes.data, r["count"].ctypes.data, r["sums"].ctypes.data,
                                r["moments"].ctypes.data if mom else None, len(r["count"]))
    for bad in (np.nan, np.inf):                                                    # a non-finite value in the pose
        for at in ((0, 0), (2, 3), (3, 1)):
            T = RIGID.copy()
            T[at] = bad
            p = col(T)
            after = C.c_int64(-5)
            assert L.ndt_map_transform(ndt._h, p.ctypes.data_as(dp), C.byref(after)) == INVALID_ARG and after.value == -5
            assert L.ndt_map_import_state_posed(*args(rec), p.ctypes.data_as(dp)) == INVALID_ARG
    assert unchanged()
    far = affine(np.eye(3), (2.0 ** 21 * leaf, 0.0, 0.0))                           # 2^21 leaves along x
    assert code_of(pkg, pkg.mapTransform, ndt, far) == GRID_OVERFLOW
    assert str(n) in L.ndt_last_error(ndt._h).decode()                              # every voxel leaves the range
    assert unchanged()
    assert code_of(pkg, pkg.mapImportStatePosed, ndt, dict(rec, leaf=leaf), far) == GRID_OVERFLOW
    assert "40" in L.ndt_last_error(ndt._h).decode()
    blow = affine(np.diag([1e300, 1.0, 1.0]), (0.0, 0.0, 0.0))                      # a centroid that is not finite
    assert code_of(pkg, pkg.mapTransform, ndt, blow) == GRID_OVERFLOW and unchanged()
    assert code_of(pkg, pkg.mapImportStatePosed, ndt, dict(rec, leaf=1.0), RIGID) == INVALID_ARG       # a wrong leaf
    assert code_of(pkg, pkg.mapImportStatePosed, ndt, dict(rec, leaf=leaf, moments=None), RIGID) == INVALID_ARG   # missing moments
    zero = dict(rec, count=rec["count"].copy())
    zero["count"][[3, 17]] = (0, -2)
    assert code_of(pkg, pkg.mapImportStatePosed, ndt, dict(zero, leaf=leaf), RIGID) == INVALID_ARG     # count < 1
    assert "2 record" in L.ndt_last_error(ndt._h).decode()
    assert unchanged()
    pkg.mapImportStatePosed(ndt, dict(rec, leaf=leaf), RIGID)                            # ... and the same records are taken
    assert states_equal(ndt.mapExportState(), repose_numpy(rec, RIGID, leaf, into=st))


# ---- 9. the rest of the handle is left alone -----------------------------------------------------------------------------
def test_the_rest_of_the_handle_is_left_alone(pkg, S):
    leaf = 1.0
    cfg = S.config_c1(max_points=10000)
    ndt = build(pkg, leaf, [cfg["target"]], capacity=0)
    ndt.setInputTargetFromMapMoments()
    ndt.setInputSource(cfg["source"])
    ndt.putKeyframe(7, cfg["source"][:500])
    T = ndt.align(cfg["guess"])
    pose6 = [0.1, -0.05, 0.02, 0.01, -0.005, 0.008]

    def state():
        h = ndt.getIterationHistory()
        return (leaf_bytes(pkg, ndt), ndt.sourceSize(), [a.tobytes() for a in h], ndt.getTiming()["n_eval_launches"],
                ndt.keyframeCount(), ndt.getFinalTransformation().tobytes())

    before, words = state(), None
    st = ndt.mapExportState()
    pkg.mapTransform(ndt, RIGID)
    pkg.mapImportStatePosed(ndt, st, np.linalg.inv(RIGID))
    assert state() == before
    words = eval_words(pkg, ndt, pose6)                                             # the target made before the transform ...
    ref = build(pkg, leaf, [cfg["target"]], capacity=0)
    ref.setInputTargetFromMapMoments()
    ref.setInputSource(cfg["source"])
    assert np.array_equal(words, eval_words(pkg, ref, pose6))                       # ... scores to the same bits
    assert np.array_equal(ndt.align(cfg["guess"]), T)


# ---- 10. hand-off modes ---------------------------------------------------------------------------------------------------
def test_transform_behind_a_deferred_build_in_both_handoff_modes(pkg, S):
    leaf = 1.0
    cfg = S.config_c1(max_points=10000)
    extra, _ = scene("small", leaf, seed=11)
    sub = mapstate_numpy(scene("small", leaf, seed=12)[0], leaf)                     # a submap's records, merged under SHIFT
    SHIFT = np.linalg.inv(RIGID)
    out = []
    for mode in (pkg.HANDOFF_SYNC, pkg.HANDOFF_ASYNC):
        ndt = engine(pkg, leaf)
        ndt.setHandoffMode(mode)
        ndt.mapReset(leaf, initial_capacity=64)
        ndt.mapEnableMoments()
        ndt.mapAdd(extra)
        ndt.setInputSource(cfg["source"])
        ndt.setInputTarget(cfg["target"])                                           # async: the build is pending
        after = pkg.mapTransform(ndt, RIGID)
        pkg.mapImportStatePosed(ndt, dict(sub, leaf=leaf), SHIFT)
        T = ndt.align(cfg["guess"])
        res = ndt.getResult()
        out.append((after, T.tobytes(), res["iterations"], res["converged"], ndt.mapExportState()))
    assert out[0][:4] == out[1][:4] and out[0][3]
    assert states_equal(out[0][4], out[1][4])
    assert states_equal(out[0][4], repose_numpy(sub, SHIFT, leaf, into=repose_numpy(mapstate_numpy(extra, leaf), RIGID, leaf)))


# ---- 11. end to end -------------------------------------------------------------------------------------------------------
def test_align_on_a_reposed_map(pkg, S):
    """Measured on an MI355X: the reposed map ends 0.0085 m / 0.00007 rad from T . gt (713 leaves), the map fed T . target
    0.0023 m / 0.00006 rad (765 leaves); the gap between the two final poses, 1.07e-2 m and 4.6e-5 rad, is the cost of
    re-binning Gaussians by their mean on this scene.  The bound is the reference tolerance smoke() uses."""
    cfg = S.config_c1(max_points=10000)
    kw = dict(step_size=0.1, trans_epsilon=1e-4, max_iterations=50)
    a = build(pkg, 1.0, [cfg["target"]], capacity=0, **kw)
    pkg.mapTransform(a, RIGID)
    b = engine(pkg, 1.0, **kw)
    b.mapReset(1.0)
    b.mapEnableMoments()
    b.mapAdd(cfg["target"], pose=RIGID)                                             # the yardstick: fed T . target directly
    finals = []
    for ndt in (a, b):
        ndt.setInputTargetFromMapMoments()
        ndt.setInputSource(cfg["source"])
        finals.append(ndt.align(RIGID @ np.asarray(cfg["guess"], np.float64)))
        assert ndt.getResult()["converged"]
    gt = RIGID @ np.asarray(cfg["gt"], np.float64)
    err = [S.pose_error(T, gt) for T in finals]
    gap = S.pose_error(finals[0], finals[1])
    print("reposed map vs gt %.4f m %.5f rad | direct map vs gt %.4f m %.5f rad | gap %.3e m %.3e rad | leaves %d vs %d"
          % (err[0] + err[1] + gap + (a.getGridInfo()["n_leaves"], b.getGridInfo()["n_leaves"])))
    assert err[1][0] < 0.05 and err[1][1] < 0.035                                   # the reference tolerance of smoke()
    assert err[0][0] < 0.05 and err[0][1] < 0.035


# ---- 12. the C++ adapter ----------------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, tmp_path):
    """tests/cpp/test_map_repose.cpp against the API mocks, built with the g++ line tests/cpp/Makefile uses for them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "tests", "cpp")
    exe = str(tmp_path / "test_map_repose")
    lib = os.path.join(root, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(root, "include", "compat"), "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(d, "test_map_repose.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "map repose: PASS" in p.stdout
