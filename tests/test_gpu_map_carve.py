"""Free-space carving of the voxel map (ndt_map_carve, ndt_map_carve_device, ndt_map_carve_keyframe) against
`carve_numpy`, the NumPy restatement of the header's rules 1-5 in tests/test_map_carve_cpu.py (which checks it against
hand-worked rays and a one-ray-at-a-time walk).  Every comparison is exact: the marks are integer counts of voxels on a
path that both sides compute with the same f64 operations in the same order, and the survivors are the table's own
records, moved; so the exported state (ijk, count, sums4, moments9) is compared with np.array_equal on the bits, and
every field of the result and of ndt_map_get_info with ==.
Shapes: the scene of that file (96 x 32 = 3072 rays from one origin towards a ground plane, a wall and a box in front of
it, leaf 0.5) plus 3000 points of `dust` between the sensor and the wall, so that a few thousand voxels lie on the rays'
paths with miss counts from 1 to some tens; scans of 37 (below one wave), 1000, 1001 and 2500 rays (no multiple of 64)
and the whole 3072 (12 blocks)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_map_target import code_of, engine, eval_words, leaf_bytes
from test_map_carve_cpu import (DEFAULTS, SCENE_LEAF, carve_numpy, carve_scene, result_of, scene_voxels)
from test_map_state_cpu import filter_state, states_equal
from test_map_target_cpu import host_transform_f64

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
LEAF = SCENE_LEAF


def pow2_at_least(v):
    c = 64
    while c < v:
        c <<= 1
    return c


def pose_of(yaw, pitch, t):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    T[:3, 3] = t
    return T


POSES = {
    "none": None,
    "near": pose_of(0.4, 0.05, [3.0, -2.0, 0.7]),
    "km": pose_of(-2.1, -0.03, [1234.5, -2345.25, 56.0]),         # a rotation and a kilometre-scale translation
    # a quarter turn and whole voxels a kilometre away: the scene stays aligned with the grid as its geometry needs it
    "quarter": np.array([[0.0, -1.0, 0.0, 1234.5], [1.0, 0.0, 0.0, -2345.0], [0.0, 0.0, 1.0, 56.0], [0.0, 0.0, 0.0, 1.0]]),
}


@pytest.fixture(scope="module")
def scene():
    sc = carve_scene()
    rng = np.random.default_rng(17)
    sc["dust"] = rng.uniform([1.0, -6.0, -1.4], [11.0, 6.0, 3.0], (3000, 3)).astype(np.float32)
    sc["inten"] = [rng.uniform(0, 255, len(s)).astype(np.float32) for s in (sc["scans"][0], sc["dust"])]
    return sc


def build(pkg, pieces, pose=None, moments=True, intensities=None, capacity=0):
    ndt = engine(pkg, LEAF)
    ndt.mapReset(LEAF, with_intensity=intensities is not None, initial_capacity=capacity)
    if moments:
        ndt.mapEnableMoments()
    for k, piece in enumerate(pieces):
        if intensities is None:
            ndt.mapAdd(piece, pose=pose)
        else:
            ndt.mapAdd(np.concatenate([piece, intensities[k][:, None]], axis=1), intensity_column=3, pose=pose)
    return ndt


def check_carve(ndt, cloud, origin, pose, reset_cap, moments=True, call=None, leaf=LEAF, **params):
    """One carve against the restatement: result, exported state, info.  Returns (state before, restatement)."""
    before, info0 = ndt.mapExportState(), ndt.mapInfo()
    prm = dict(DEFAULTS, **params)
    want = carve_numpy(before["ijk"], before["count"], cloud, origin, leaf, pose, **prm)
    got = (call or ndt.mapCarve)(cloud, origin, pose=pose, **params)
    print("carve: %s" % got)
    assert got == result_of(want)
    keep = want["keep"]
    kept = int(keep.sum())
    after, info = ndt.mapExportState(), ndt.mapInfo()
    assert states_equal(after, filter_state(before, keep), moments=moments)
    assert info["n_voxels"] == kept and info["n_points"] == int(before["count"][keep].sum())
    if want["n_removed"] == 0:
        assert info == info0                                                                   # the table is untouched
    else:
        assert info["capacity"] == max(pow2_at_least(2 * kept), reset_cap)
        if kept:
            assert info["min_ijk"] == tuple(before["ijk"][keep].min(0)) and info["max_ijk"] == tuple(before["ijk"][keep].max(0))
    for k in ("n_points_dropped", "n_adds", "n_grows", "leaf", "with_intensity"):
        assert info[k] == info0[k], k
    return before, want


# ---- 1. exact survivors -------------------------------------------------------------------------------------------------
#        name: (pose, moments, intensity, rays, parameters)
EXACT = {
    "defaults": ("none", True, False, 3072, {}),
    "km-misses1": ("km", False, True, 1000, dict(min_misses=1, keep_last=0)),
    "near-misses5": ("near", True, False, 1001, dict(min_misses=5, keep_last=3)),
    "km-truncated": ("km", True, True, 2500, dict(min_misses=2, keep_last=1, max_steps=6)),
    "protected": ("none", False, False, 1000, dict(min_misses=1, keep_last=1, protect_min_count=2)),
    "below-a-wave": ("near", True, False, 37, dict(min_misses=1, keep_last=0)),
    "misses2-keep3": ("none", True, False, 1001, dict(min_misses=2, keep_last=3)),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_survivors_are_exactly_the_restatements(pkg, scene, name):
    pose_name, moments, inten, n, params = EXACT[name]
    pose = POSES[pose_name]
    ndt = build(pkg, [scene["scans"][0], scene["dust"]], pose, moments, scene["inten"] if inten else None)
    pick = np.random.default_rng(len(name)).permutation(len(scene["scans"][2]))[:n]
    cloud = scene["scans"][2][np.sort(pick)].copy()
    if n >= 1000:                                                 # skipped rays among the others
        cloud[5] = np.nan
        cloud[77, 2] = np.inf
        cloud[300] = [6e5, 0.0, 0.0]                              # voxel 1.2e6 without a pose
        cloud[301] = [0.0, -3e6, 0.0]
    before, want = check_carve(ndt, cloud, scene["origin"], pose, 1 << 18, moments, **params)
    assert 0 < want["n_removed"] < len(before["count"]) and want["n_voxels_hit"] > 0
    if n >= 1000:
        assert want["n_rays_skipped"] >= 3
    if "max_steps" in params:                                     # most rays are cut short
        full = carve_numpy(before["ijk"], before["count"], cloud, scene["origin"], LEAF, pose, **dict(DEFAULTS, **dict(params, max_steps=200)))
        assert want["n_steps"] < full["n_steps"] // 2
    if "protect_min_count" in params:
        free = carve_numpy(before["ijk"], before["count"], cloud, scene["origin"], LEAF, pose, **dict(DEFAULTS, **dict(params, protect_min_count=0)))
        assert want["n_removed"] < free["n_removed"]
    # the same scan again: what it looks through is gone already, the rest took a hit or too few misses -- and still
    # whatever happens is the restatement's
    check_carve(ndt, cloud, scene["origin"], pose, 1 << 18, moments, **params)


# ---- 2. dry runs ----------------------------------------------------------------------------------------------------------
def test_dry_runs_count_and_change_nothing(pkg, scene):
    pose = POSES["near"]
    ndt = build(pkg, [scene["scans"][0], scene["dust"]], pose)
    before, info0 = ndt.mapExportState(), ndt.mapInfo()
    cloud, origin = scene["scans"][2][:1500], scene["origin"]
    want = carve_numpy(before["ijk"], before["count"], cloud, origin, LEAF, pose, **DEFAULTS)
    open_to_carving = want["misses"][~want["hit"]]
    top = int(open_to_carving.max())
    assert top >= 8
    hist = {}
    for mm in (1, 2, 3, 5, 8, top, top + 1):
        got = ndt.mapCarve(cloud, origin, pose=pose, min_misses=mm, dry_run=True)
        assert got == result_of(carve_numpy(before["ijk"], before["count"], cloud, origin, LEAF, pose, **dict(DEFAULTS, min_misses=mm)))
        hist[mm] = got["n_removed"]
        assert ndt.mapInfo() == info0
    # the miss histogram of the voxels without a hit, cumulated from above
    assert hist == {mm: int((open_to_carving >= mm).sum()) for mm in hist}
    assert hist[top + 1] == 0 < hist[top] <= hist[8] < hist[1]
    assert states_equal(ndt.mapExportState(), before)
    real = ndt.mapCarve(cloud, origin, pose=pose)                                    # the real run reports what the dry run did
    assert real == result_of(want) and ndt.mapInfo()["n_voxels"] == info0["n_voxels"] - hist[2]


# ---- 3. the scene ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose_name", ["none", "quarter"])
def test_scene_the_car_goes_wall_and_ground_stay(pkg, scene, pose_name):
    pose = POSES[pose_name]
    ndt = build(pkg, scene["scans"][:2], pose)
    before, want = check_carve(ndt, scene["scans"][2], scene["origin"], pose, 1 << 18)
    car, wall, ground = scene_voxels(scene, pose)
    removed = set(map(tuple, before["ijk"][~want["keep"]]))
    left = set(map(tuple, ndt.mapExportState()["ijk"]))
    assert len(car) >= 10 and removed == car and not (left & car)                  # all car voxels go
    assert wall <= left and ground <= left                                         # every wall and ground voxel is kept
    # without keep_last the grazing rays would have taken ground voxels too (a dry run on what is left of the map)
    st = ndt.mapExportState()
    graze = carve_numpy(st["ijk"], st["count"], scene["scans"][2], scene["origin"], LEAF, pose, **dict(DEFAULTS, keep_last=0))
    assert ndt.mapCarve(scene["scans"][2], scene["origin"], pose=pose, keep_last=0, dry_run=True) == result_of(graze)
    assert len(set(map(tuple, st["ijk"][~graze["keep"]])) & ground) >= 10


# ---- 4. continuity ---------------------------------------------------------------------------------------------------------
def test_carve_then_add_and_target_from_the_survivors(pkg, scene):
    pose = POSES["near"]
    ndt = build(pkg, [scene["scans"][0], scene["dust"]], pose, capacity=64)
    before, want = check_carve(ndt, scene["scans"][2], scene["origin"], pose, 64, min_misses=1)
    survivors = filter_state(before, want["keep"])
    fresh = engine(pkg, LEAF)
    fresh.mapReset(LEAF)
    fresh.mapEnableMoments()
    fresh.mapImportState(dict(leaf=LEAF, **survivors))
    # targets made from the moments: the leaves of the surviving voxels
    ndt.setInputTargetFromMapMoments()
    fresh.setInputTargetFromMapMoments()
    gi = ndt.getGridInfo()
    assert gi["n_leaves"] > 50 and gi["n_target_points"] == int(survivors["count"].sum())
    assert leaf_bytes(pkg, ndt) == leaf_bytes(pkg, fresh)
    # both go on with the same add (the second scan brings voxels the carve removed, voxels that stayed and new ones)
    for e in (ndt, fresh):
        e.mapAdd(scene["scans"][1], pose=pose)
    a, b = ndt.mapExportState(), fresh.mapExportState()
    assert states_equal(a, b) and len(a["count"]) > len(survivors["count"])
    ia, ib = ndt.mapInfo(), fresh.mapInfo()
    for k in ("n_voxels", "n_points", "min_ijk", "max_ijk"):
        assert ia[k] == ib[k], k


# ---- 5. the three forms ---------------------------------------------------------------------------------------------------
def test_host_device_and_keyframe_forms_agree(pkg, scene, hipmem):
    pose, origin = POSES["km"], scene["origin"]
    cloud = scene["scans"][2][:2001].copy()
    cloud[9] = np.nan
    maps = [build(pkg, [scene["scans"][0], scene["dust"]], pose) for _ in range(3)]
    before = maps[0].mapExportState()
    want = carve_numpy(before["ijk"], before["count"], cloud, origin, LEAF, pose, **DEFAULTS)
    dx, dy, dz = (hipmem.upload(np.ascontiguousarray(cloud[:, a])) for a in range(3))
    maps[2].putKeyframe(4, cloud)
    results = [maps[0].mapCarve(cloud, origin, pose=pose),
               maps[1].mapCarveDevice(dx, dy, dz, len(cloud), origin, pose=pose),
               maps[2].mapCarveKeyframe(4, origin, pose)]
    assert results[0] == results[1] == results[2] == result_of(want) and want["n_removed"] > 0 and want["n_rays_skipped"] == 1
    states = [m.mapExportState() for m in maps]
    assert states_equal(states[0], filter_state(before, want["keep"]))
    assert states_equal(states[0], states[1]) and states_equal(states[0], states[2])
    assert maps[0].mapInfo() == maps[1].mapInfo() == maps[2].mapInfo()
    assert maps[2].keyframeCount() == 1
    # a padded host cloud (stride 16) is the same cloud
    again = build(pkg, [scene["scans"][0], scene["dust"]], pose)
    padded = np.concatenate([cloud, np.full((len(cloud), 1), 7.0, np.float32)], axis=1)
    assert again.mapCarve(padded, origin, pose=pose) == results[0] and states_equal(again.mapExportState(), states[0])


# ---- 6. edges ---------------------------------------------------------------------------------------------------------------
def test_edges_skipped_rays_no_rays_nothing_to_remove_everything_to_remove(pkg, scene):
    origin = scene["origin"]
    ndt = build(pkg, [scene["scans"][0], scene["dust"]], capacity=64)               # a table that grew
    before, info0 = ndt.mapExportState(), ndt.mapInfo()
    assert info0["n_grows"] >= 1 and info0["capacity"] > 64
    zero = dict(n_rays=0, n_rays_skipped=0, n_steps=0, n_voxels_crossed=0, n_voxels_hit=0, n_removed=0, n_points_removed=0)
    assert ndt.mapCarve(np.zeros((0, 3), np.float32), origin) == zero               # n = 0
    assert ndt.mapCarveDevice(None, None, None, 0, origin) == zero
    # nothing but skipped rays: not finite, beyond 2^20 voxels, not finite behind the pose
    bad = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [6e5, 0, 0], [0, -524287.75, 0], [3e38, 3e38, 0]])
    assert ndt.mapCarve(bad, origin) == dict(zero, n_rays=6, n_rays_skipped=6)
    got = ndt.mapCarve(bad, origin, pose=np.diag([2.0, 2.0, 2.0, 1.0]))            # (a pose that doubles: 6e38 is not an f32)
    assert got == dict(zero, n_rays=6, n_rays_skipped=6)
    # an origin beyond the coordinate range skips every ray
    assert ndt.mapCarve(scene["scans"][2][:100], [6e5, 0.0, 0.0]) == dict(zero, n_rays=100, n_rays_skipped=100)
    # a carve that removes nothing leaves the table as it is, grown capacity included
    _, want = check_carve(ndt, scene["scans"][2], origin, None, 64, min_misses=100000)
    assert want["n_removed"] == 0 and want["n_voxels_crossed"] > 1000
    assert ndt.mapInfo() == info0 and states_equal(ndt.mapExportState(), before)
    # after a crop: the sliding window first, then the scan
    lo, hi = [0.0, -4.0, -2.0], [9.0, 4.0, 2.0]
    assert ndt.mapCrop(lo, hi) > 0
    cropped, want = check_carve(ndt, scene["scans"][2], origin, None, 64, min_misses=3)
    assert 0 < want["n_removed"] < len(cropped["count"]) < len(before["count"])
    # a carve that empties the map: a map of the rays' midpoints alone, every one looked through
    mid = ((scene["scans"][2].astype(np.float64) + origin) / 2).astype(np.float32)
    ndt = build(pkg, [mid], capacity=64)
    info0 = ndt.mapInfo()
    before, want = check_carve(ndt, scene["scans"][2], origin, None, 64, min_misses=1, keep_last=0)
    assert want["n_removed"] == len(before["count"]) == info0["n_voxels"] and want["n_points_removed"] == len(mid)
    info = ndt.mapInfo()
    assert info["n_voxels"] == 0 and info["n_points"] == 0 and info["capacity"] == 64 and ndt.mapHasMoments()
    assert len(ndt.mapExportState()["count"]) == 0
    _, again = check_carve(ndt, scene["scans"][2], origin, None, 64, min_misses=1, keep_last=0)   # rays through an empty map
    assert again["n_steps"] == want["n_steps"] > 0 and again["n_voxels_crossed"] == again["n_voxels_hit"] == 0
    ndt.mapAdd(mid)                                                                 # the emptied map goes on
    assert states_equal(ndt.mapExportState(), before)


def test_refusals_change_nothing(pkg, scene):
    L = pkg.lib()
    origin = scene["origin"]
    ndt = engine(pkg, LEAF)
    cloud = scene["scans"][2][:500]
    assert code_of(pkg, ndt.mapCarve, cloud, origin) == INVALID_ARG                 # no map
    ndt = build(pkg, [scene["scans"][0]])
    before, info0 = ndt.mapExportState(), ndt.mapInfo()
    bad_pose = np.eye(4)
    bad_pose[1, 3] = np.nan
    assert code_of(pkg, ndt.mapCarve, cloud, origin, pose=bad_pose) == INVALID_ARG
    assert code_of(pkg, ndt.mapCarveKeyframe, 99, origin, np.eye(4)) == INVALID_ARG            # unknown keyframe
    assert code_of(pkg, ndt.mapCarve, cloud, [3e38, 0.0, 0.0], pose=np.diag([2.0, 2.0, 2.0, 1.0])) == INVALID_ARG   # origin behind the pose
    # at the C boundary (the Python mirror refuses these before the library)
    prm = pkg.MapCarveParams()
    L.ndt_map_carve_default_params(C.byref(prm))
    res = pkg.MapCarveResult(7, 7, 7, 7, 7, 7, 7)
    fp = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    o = np.ascontiguousarray(origin, np.float32)
    c = np.ascontiguousarray(cloud)
    assert L.ndt_map_carve(ndt._h, c.ctypes.data, len(c), 12, None, None, C.byref(prm), C.byref(res)) == INVALID_ARG
    assert L.ndt_map_carve(ndt._h, c.ctypes.data, len(c), 12, fp(o), None, None, C.byref(res)) == INVALID_ARG
    for field, value in (("min_misses", 0), ("keep_last", -1), ("max_steps", 0), ("max_steps", 65537), ("protect_min_count", -1)):
        p = pkg.MapCarveParams()
        L.ndt_map_carve_default_params(C.byref(p))
        setattr(p, field, value)
        assert L.ndt_map_carve(ndt._h, c.ctypes.data, len(c), 12, fp(o), None, C.byref(p), C.byref(res)) == INVALID_ARG, field
    prm.reserved[2] = 5
    assert L.ndt_map_carve(ndt._h, c.ctypes.data, len(c), 12, fp(o), None, C.byref(prm), C.byref(res)) == INVALID_ARG
    assert res.n_rays == 7 and res.n_removed == 7
    assert ndt.mapInfo() == info0 and states_equal(ndt.mapExportState(), before)
    # a NULL result pointer is allowed
    prm.reserved[2] = 0
    assert L.ndt_map_carve(ndt._h, c.ctypes.data, len(c), 12, fp(o), None, C.byref(prm), None) == 0
    ndt.mapClear()
    assert code_of(pkg, ndt.mapCarve, cloud, origin) == INVALID_ARG                 # after mapClear: no map again


# ---- 7. the rest of the handle is left alone ----------------------------------------------------------------------------
def test_the_rest_of_the_handle_is_left_alone(pkg, scene):
    origin = scene["origin"]
    ndt = build(pkg, [scene["scans"][0], scene["scans"][1]])
    ndt.setInputTargetFromMapMoments()                                             # a target made from this very map
    ndt.setInputSource(scene["scans"][2])
    ndt.putKeyframe(7, scene["scans"][0])
    ndt.align(np.eye(4))
    p = np.array([0.05, -0.03, 0.02, 0.01, -0.005, 0.008])
    words = eval_words(pkg, ndt, p)

    def state():
        h = ndt.getIterationHistory()
        return (leaf_bytes(pkg, ndt), ndt.sourceSize(), [a.tobytes() for a in h], ndt.getTiming()["n_eval_launches"],
                ndt.keyframeCount(), ndt.getFinalTransformation().tobytes(), ndt.getGridInfo()["n_target_points"])

    before = state()
    _, want = check_carve(ndt, scene["scans"][2], origin, None, 1 << 18)
    assert want["n_removed"] > 0
    assert ndt.mapCarveKeyframe(7, origin, np.eye(4), dry_run=True)["n_rays"] == len(scene["scans"][0])
    assert state() == before
    assert np.array_equal(eval_words(pkg, ndt, p), words)


# ---- 8. the C++ adapter -----------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, tmp_path):
    """tests/cpp/test_map_carve.cpp against the API mocks, built with the g++ line tests/cpp/Makefile uses for them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "tests", "cpp")
    exe = str(tmp_path / "test_map_carve")
    lib = os.path.join(root, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(root, "include", "compat"), "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(d, "test_map_carve.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "map carve: PASS" in p.stdout
