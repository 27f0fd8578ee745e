"""CPU checks of the free-space carving boundary (ndt_map_carve_default_params, ndt_map_carve, ndt_map_carve_device,
ndt_map_carve_keyframe; no GPU): the four symbols are declared with their parameter lists, exported, listed and bound,
the defaults are 2, 1, 4096, 0, 0; NULL and out-of-range arguments are refused before the handle is looked at; the kernels
of ndt_map_carve.hip compile for gfx950 without scratch, with integer atomics only and no inline assembly.
The yardstick the GPU tests compare with lives here: `carve_numpy`, a NumPy restatement of rules 1-5 of the header
comment (frame, skipped rays, the Amanatides-Woo walk in f64 with every operation rounded as written, marks, removal),
vectorised over the rays.  It is checked against `walk`, the same rules written one ray at a time in plain Python floats,
on hand-worked rays and on random ones, and every voxel of a path is shown to touch its segment."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_map_state_cpu import state_key
from test_map_target_cpu import host_transform_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_map_carve_default_params", "ndt_map_carve_device", "ndt_map_carve", "ndt_map_carve_keyframe")
LIMIT = 1 << 20
DEFAULTS = dict(min_misses=2, keep_last=1, max_steps=4096, protect_min_count=0)


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def to_grid(p, leaf):
    """(double)(p_f32 * inv_leaf_f32) per axis: the f32 product ndt_map_add floors, widened"""
    inv = np.float32(1.0) / np.float32(leaf)
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(p, np.float32) * inv).astype(np.float64)


def walk(gs, ge):
    """Rule 3 for one ray in plain Python floats (IEEE f64): the path [v_0 = floor(gs), ..., v_L = floor(ge)]."""
    gs, ge = [float(v) for v in gs], [float(v) for v in ge]
    v = [int(np.floor(g)) for g in gs]
    ve = [int(np.floor(g)) for g in ge]
    inf = float("inf")
    step, tdelta, tmax = [0] * 3, [0.0] * 3, [inf] * 3
    for a in range(3):
        if ve[a] != v[a]:
            d = ge[a] - gs[a]
            step[a] = 1 if ve[a] > v[a] else -1
            tdelta[a] = 1.0 / abs(d)
            tmax[a] = (float(v[a] + (1 if step[a] > 0 else 0)) - gs[a]) / d
    path = [tuple(v)]
    for _ in range(sum(abs(ve[a] - v[a]) for a in range(3))):
        a = 0 if tmax[0] <= tmax[1] and tmax[0] <= tmax[2] else 1 if tmax[1] <= tmax[2] else 2   # the lowest axis on equal values
        v[a] += step[a]
        tmax[a] = inf if v[a] == ve[a] else tmax[a] + tdelta[a]
        path.append(tuple(v))
    assert list(path[-1]) == ve
    return path


def ray_marks(path, keep_last, max_steps):
    """Rule 4 for one path: (the voxels that take a miss, the voxel that takes the hit)"""
    bound = max(0, min(len(path) - 1 - 1 - keep_last, max_steps))
    return path[1:1 + bound], path[-1]


def carve_numpy(ijk, count, pts, origin, leaf, pose=None, min_misses=2, keep_last=1, max_steps=4096, protect_min_count=0):
    """Rules 1-5 for one call on a map that holds the voxels `ijk` [m, 3] with `count` [m] points: dict with every field of
    ndt_map_carve_result, `misses` [m] and `hit` [m] (the marks per voxel) and `keep` [m] (the voxels that stay)."""
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    count = np.asarray(count, np.int64)
    p = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 3))
    o = np.asarray(origin, np.float32).reshape(1, 3)
    n = len(p)
    fin = np.isfinite(p).all(axis=1)
    if pose is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            p, o = host_transform_f64(np.asarray(pose, np.float64), p), host_transform_f64(np.asarray(pose, np.float64), o)
        fin &= np.isfinite(p).all(axis=1)
    assert np.isfinite(o).all()
    gs, ge = to_grid(o, leaf)[0], to_grid(p, leaf)
    with np.errstate(invalid="ignore"):
        fs, fe = np.floor(gs), np.floor(ge)
        ok = fin & (np.abs(fe) < LIMIT).all(axis=1) & bool((np.abs(fs) < LIMIT).all())
    ge, ve = ge[ok], fe[ok].astype(np.int64)
    r = len(ge)
    vs = fs.astype(np.int64) if r else np.zeros(3, np.int64)
    v = np.tile(vs, (r, 1))
    L = np.abs(ve - v).sum(axis=1)
    bound = np.clip(np.minimum(L - 1 - keep_last, max_steps), 0, None)
    moving = ve != v
    with np.errstate(divide="ignore", invalid="ignore"):
        d = ge - gs
        step = np.where(ve > v, 1, -1)
        tdelta = np.where(moving, 1.0 / np.abs(d), 0.0)
        tmax = np.where(moving, ((v + (step > 0)).astype(np.float64) - gs) / d, np.inf)
    missed = []
    rows = np.arange(r)
    for k in range(int(bound.max()) if r else 0):
        act = rows[bound > k]
        a = np.argmin(tmax[act], axis=1)                    # the first minimum: the lowest axis on equal values
        v[act, a] += step[act, a]
        done = v[act, a] == ve[act, a]
        tmax[act, a] = np.where(done, np.inf, tmax[act, a] + tdelta[act, a])
        missed.append(state_key(v[act]))
    keys = state_key(ijk)
    order = np.argsort(keys)

    def per_voxel(marked):
        """how often each voxel of the map appears among the marked keys"""
        out = np.zeros(len(keys), np.int64)
        if len(keys) and len(marked):
            u, c = np.unique(marked, return_counts=True)
            at = np.searchsorted(keys[order], u)
            at[at == len(keys)] = 0
            found = keys[order][at] == u
            out[order[at[found]]] = c[found]
        return out

    misses = per_voxel(np.concatenate(missed) if missed else np.zeros(0, np.int64))
    hit = per_voxel(state_key(ve)) > 0
    remove = (misses >= min_misses) & ~hit
    if protect_min_count > 0:
        remove &= count < protect_min_count
    return dict(n_rays=n, n_rays_skipped=n - r, n_steps=int(bound.sum()), n_voxels_crossed=int((misses > 0).sum()),
                n_voxels_hit=int(hit.sum()), n_removed=int(remove.sum()), n_points_removed=int(count[remove].sum()),
                misses=misses, hit=hit, keep=~remove)


RESULT_FIELDS = ("n_rays", "n_rays_skipped", "n_steps", "n_voxels_crossed", "n_voxels_hit", "n_removed", "n_points_removed")


def result_of(want):
    return {k: want[k] for k in RESULT_FIELDS}


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, fp, dp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double)
    pp, rp = C.POINTER(pkg.MapCarveParams), C.POINTER(pkg.MapCarveResult)
    want = {
        "ndt_map_carve_default_params": [pp],
        "ndt_map_carve_device": [vp, vp, vp, vp, C.c_size_t, fp, dp, pp, rp],
        "ndt_map_carve": [vp, vp, C.c_size_t, C.c_size_t, fp, dp, pp, rp],
        "ndt_map_carve_keyframe": [vp, C.c_int64, fp, dp, pp, rp],
    }
    for name in NEW:
        assert re.search(r"\b(int|void) %s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    assert L.ndt_map_carve_default_params.restype is None
    # the declared parameter lists: types in order, whatever the parameters are called
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))

    def types_of(name):
        args = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, flat).group(1).split(",")
        out = []
        for a in args:
            a = a.strip()
            arr = re.search(r"\[(\d+)\]$", a)
            a = re.sub(r"\[\d+\]$", "", a)
            a = re.sub(r"\s*\b[a-z_0-9]+$", "", a) if not a.endswith("*") else a        # drop the parameter's name
            out.append(a.replace(" *", "*") + ("[%s]" % arr.group(1) if arr else ""))
        return out

    assert types_of("ndt_map_carve_default_params") == ["ndt_map_carve_params*"]
    assert types_of("ndt_map_carve_device") == ["ndt_handle*", "const float*", "const float*", "const float*", "size_t",
                                                "const float[3]", "const double*", "const ndt_map_carve_params*",
                                                "ndt_map_carve_result*"]
    assert types_of("ndt_map_carve") == ["ndt_handle*", "const float*", "size_t", "size_t", "const float[3]", "const double*",
                                         "const ndt_map_carve_params*", "ndt_map_carve_result*"]
    assert types_of("ndt_map_carve_keyframe") == ["ndt_handle*", "int64_t", "const float[3]", "const double[16]",
                                                  "const ndt_map_carve_params*", "ndt_map_carve_result*"]
    assert ("typedef struct ndt_map_carve_params { int min_misses; int keep_last; int max_steps; int protect_min_count; "
            "int dry_run; int reserved[3]; } ndt_map_carve_params;") in flat
    assert ("typedef struct ndt_map_carve_result { int64_t n_rays, n_rays_skipped, n_steps, n_voxels_crossed, n_voxels_hit, "
            "n_removed, n_points_removed; } ndt_map_carve_result;") in flat
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    assert C.sizeof(pkg.MapCarveParams) == 32 and C.sizeof(pkg.MapCarveResult) == 56
    assert [f for f, _ in pkg.MapCarveResult._fields_] == list(RESULT_FIELDS)
    # the declarations follow the crop block
    assert hdr.index("int ndt_map_crop(") < hdr.index("typedef struct ndt_map_carve_params") < hdr.index("ndt_set_regularization_pose")
    hpp = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    for m in ("mapCarve", "mapCarveDevice", "mapCarveKeyframe"):
        assert callable(getattr(pkg.NormalDistributionsTransform, m)), m
        assert re.search(r"\b%s\s*\(" % m, hpp), m
    assert hpp.index("mapCrop(") < hpp.index("mapCarve(")


def test_defaults(pkg):
    L = pkg.lib()
    p = pkg.MapCarveParams(9, 9, 9, 9, 9, (9, 9, 9))
    L.ndt_map_carve_default_params(C.byref(p))
    assert (p.min_misses, p.keep_last, p.max_steps, p.protect_min_count, p.dry_run) == (2, 1, 4096, 0, 0)
    assert list(p.reserved) == [0, 0, 0]
    L.ndt_map_carve_default_params(None)                                                      # (nothing to write: no crash)
    assert DEFAULTS == dict(min_misses=2, keep_last=1, max_steps=4096, protect_min_count=0)


def test_argument_errors_come_before_the_handle(pkg):
    L = pkg.lib()
    n_dev, _ = pkg.backend_info()
    if n_dev <= 0:
        with pytest.raises(pkg.NdtError) as ei:
            pkg.NormalDistributionsTransform().mapCarve(np.zeros((4, 3), np.float32), [0.0, 0.0, 0.0])
        assert ei.value.code == -2                           # NDT_ERR_NO_DEVICE: no CPU fallback
    f = (C.c_float * 64)()
    origin = (C.c_float * 3)(0.0, 0.0, 0.0)
    pose = (C.c_double * 16)(*np.eye(4).ravel())
    res = pkg.MapCarveResult(7, 7, 7, 7, 7, 7, 7)
    good = pkg.MapCarveParams()
    L.ndt_map_carve_default_params(C.byref(good))

    def forms(h, org, prm):
        return (L.ndt_map_carve(h, f, 4, 12, org, None, prm, C.byref(res)),
                L.ndt_map_carve_device(h, f, f, f, 4, org, None, prm, C.byref(res)),
                L.ndt_map_carve_keyframe(h, 1, org, pose, prm, C.byref(res)))

    assert forms(None, origin, C.byref(good)) == (-1, -1, -1)                                  # NULL handle
    # the argument checks come before the handle is looked at: a stand-in block of zero bytes is never read
    h = C.create_string_buffer(1 << 16)
    assert forms(h, None, C.byref(good)) == (-1, -1, -1)                                       # NULL origin
    assert forms(h, origin, None) == (-1, -1, -1)                                              # NULL params
    for bad in ((C.c_float * 3)(float("nan"), 0.0, 0.0), (C.c_float * 3)(0.0, float("inf"), 0.0),
                (C.c_float * 3)(0.0, 0.0, -float("inf"))):
        assert forms(h, bad, C.byref(good)) == (-1, -1, -1)                                    # an origin that is not finite
    for field, value in (("min_misses", 0), ("min_misses", -3), ("keep_last", -1), ("max_steps", 0), ("max_steps", 65537),
                         ("max_steps", -1), ("protect_min_count", -1)):
        p = pkg.MapCarveParams()
        L.ndt_map_carve_default_params(C.byref(p))
        setattr(p, field, value)
        assert forms(h, origin, C.byref(p)) == (-1, -1, -1), (field, value)
    for k in range(3):
        p = pkg.MapCarveParams()
        L.ndt_map_carve_default_params(C.byref(p))
        p.reserved[k] = 1
        assert forms(h, origin, C.byref(p)) == (-1, -1, -1), k
    assert L.ndt_map_carve(h, None, 4, 12, origin, None, C.byref(good), C.byref(res)) == -1    # no cloud
    for stride in (8, 14):
        assert L.ndt_map_carve(h, f, 4, stride, origin, None, C.byref(good), C.byref(res)) == -1
    assert L.ndt_map_carve_device(h, f, None, f, 4, origin, None, C.byref(good), C.byref(res)) == -1
    assert L.ndt_map_carve_keyframe(h, 1, origin, None, C.byref(good), C.byref(res)) == -1     # a keyframe needs its pose
    assert [getattr(res, k) for k in RESULT_FIELDS] == [7] * 7 and bytes(h.raw) == bytes(1 << 16)   # nothing was written


def test_python_mirror_validates_before_the_library(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)   # no handle: nothing may reach the library
    ndt._h = None
    cloud = np.zeros((4, 3), np.float32)
    bad = [
        lambda: ndt.mapCarve(cloud, [0.0, 0.0]), lambda: ndt.mapCarve(cloud, [0.0, np.nan, 0.0]),
        lambda: ndt.mapCarve(cloud, [0.0, 0.0, 0.0], min_misses=0), lambda: ndt.mapCarve(cloud, [0.0, 0.0, 0.0], keep_last=-1),
        lambda: ndt.mapCarve(cloud, [0.0, 0.0, 0.0], max_steps=0), lambda: ndt.mapCarve(cloud, [0.0, 0.0, 0.0], max_steps=65537),
        lambda: ndt.mapCarve(cloud, [0.0, 0.0, 0.0], protect_min_count=-1),
        lambda: ndt.mapCarve(np.zeros((4, 2), np.float32), [0.0, 0.0, 0.0]),
        lambda: ndt.mapCarve(cloud, [0.0, 0.0, 0.0], pose=np.eye(3)),
        lambda: ndt.mapCarveDevice(0, 0, 0, 4, [np.inf, 0.0, 0.0]),
        lambda: ndt.mapCarveKeyframe(1, [0.0, 0.0, 0.0], None),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d reached the library" % k)


# ---- the restatement against hand-worked rays -------------------------------------------------------------------------
def path_of(origin, point, leaf):
    return walk(to_grid(np.float32(origin), leaf), to_grid(np.float32(point), leaf))


def test_hand_worked_rays():
    leaf = 0.5
    # parallel to an axis: voxels (0,0,0) .. (6,0,0), one step each
    p = path_of([0.25, 0.25, 0.25], [3.25, 0.25, 0.25], leaf)
    assert p == [(i, 0, 0) for i in range(7)]
    assert ray_marks(p, 0, 4096) == ([(i, 0, 0) for i in range(1, 6)], (6, 0, 0))
    assert ray_marks(p, 1, 4096) == ([(i, 0, 0) for i in range(1, 5)], (6, 0, 0))
    assert ray_marks(p, 3, 4096) == ([(1, 0, 0), (2, 0, 0)], (6, 0, 0))
    # truncation by max_steps: the first three voxels after the start, the hit still at the end
    assert ray_marks(p, 0, 3) == ([(1, 0, 0), (2, 0, 0), (3, 0, 0)], (6, 0, 0))
    assert ray_marks(p, 1, 1) == ([(1, 0, 0)], (6, 0, 0))
    # keep_last >= L and keep_last = L - 1: no miss at all
    for keep in (5, 6, 7, 100):
        assert ray_marks(p, keep, 4096) == ([], (6, 0, 0)), keep
    # the diagonal in the plane: gs = (0.5, 0.5, 0.5), ge = (10.5, 10.5, 0.5), d = (10, 10, 0): tMax is 0.05 on x and on
    # y and both go on by the same 0.1, so every pair of steps is a tie and x, the lower axis, goes first
    p = path_of([0.25, 0.25, 0.25], [5.25, 5.25, 0.25], leaf)
    want = [(0, 0, 0)]
    for i in range(1, 11):
        want += [(i, i - 1, 0), (i, i, 0)]
    assert p == want and len(p) == 21
    # ... and in space, all three axes tied: x, then y, then z
    p = path_of([0.25, 0.25, 0.25], [1.75, 1.75, 1.75], leaf)
    assert p == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3)]
    # L = 0: the ray ends in the voxel it starts in -- no miss, the hit there
    p = path_of([0.25, 0.25, 0.25], [0.3, 0.4, 0.1], leaf)
    assert p == [(0, 0, 0)] and ray_marks(p, 0, 4096) == ([], (0, 0, 0))
    # L = 1: the neighbour takes the hit and nothing a miss, even with keep_last = 0
    p = path_of([0.25, 0.25, 0.25], [0.25, 0.75, 0.25], leaf)
    assert p == [(0, 0, 0), (0, 1, 0)] and ray_marks(p, 0, 4096) == ([], (0, 1, 0))
    # L = 2 with keep_last = 0: exactly the voxel between
    p = path_of([0.25, 0.25, 0.25], [0.25, 0.25, -0.75], leaf)
    assert p == [(0, 0, 0), (0, 0, -1), (0, 0, -2)] and ray_marks(p, 0, 4096) == ([(0, 0, -1)], (0, 0, -2))
    # negative coordinates: gs = (-0.5, -0.5, 0.5) in voxel (-1, -1, 0), ge = (-5.5, -0.5, 0.5) in (-6, -1, 0)
    p = path_of([-0.25, -0.25, 0.25], [-2.75, -0.25, 0.25], leaf)
    assert p == [(-i, -1, 0) for i in range(1, 7)]
    # negative and oblique: from (-0.25, -0.25) towards (-1.75, -0.75): gs = (-0.5, -0.5), ge = (-3.5, -1.5), d = (-3, -1)
    # tMax_x = (-1 + 0.5) / -3 = 1/6, then 1/2, 5/6; tMax_y = (-1 + 0.5) / -1 = 1/2: at 1/2 x and y tie and x goes first
    p = path_of([-0.25, -0.25, 0.25], [-1.75, -0.75, 0.25], leaf)
    assert p == [(-1, -1, 0), (-2, -1, 0), (-3, -1, 0), (-3, -2, 0), (-4, -2, 0)]


def test_the_vectorised_restatement_is_the_walk():
    rng = np.random.default_rng(5)
    leaf = 0.5
    origin = np.float32([0.3, -0.2, 1.1])
    pts = rng.uniform(-12, 12, (300, 3)).astype(np.float32)
    pts[:40] = np.round(pts[:40] * 2) / 2 + 0.25                 # voxel centres: ties
    pts[40:60, 2] = origin[2]                                    # in the plane of the origin
    pts[7] = np.nan
    pts[9, 1] = np.inf
    pts[11] = [6e6, 0.0, 0.0]                                    # voxel 1.2e7: beyond 2^20, with and without the pose
    pts[13] = [0.0, -6e6, 0.0]
    T = np.eye(4)
    c, s = np.cos(0.7), np.sin(0.7)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [1000.0, -2000.0, 5.0]
    for pose in (None, T):
        # the map: every other voxel any path visits, and two that none does
        mo = origin[None] if pose is None else host_transform_f64(pose, origin[None])
        with np.errstate(invalid="ignore"):
            mp = pts if pose is None else host_transform_f64(pose, pts)
        gs = to_grid(mo, leaf)[0]
        paths = {}
        for i, q in enumerate(mp):
            g = to_grid(q, leaf)
            if np.isfinite(pts[i]).all() and (np.abs(np.floor(g)) < LIMIT).all():
                paths[i] = walk(gs, g)
        assert len(pts) - len(paths) == 4
        vox = sorted({v for pa in paths.values() for v in pa})[::2] + [(900, 900, 900), (-900, 5, 5)]
        ijk = np.array(vox, np.int64)
        count = rng.integers(1, 9, len(ijk))
        for keep_last, max_steps, min_misses, protect in ((1, 4096, 2, 0), (0, 4096, 1, 0), (3, 7, 1, 0), (1, 4096, 2, 4)):
            got = carve_numpy(ijk, count, pts, origin, leaf, pose, min_misses, keep_last, max_steps, protect)
            miss, hit, steps = {}, set(), 0
            for pa in paths.values():
                ms, ht = ray_marks(pa, keep_last, max_steps)
                steps += len(ms)
                for v in ms:
                    miss[v] = miss.get(v, 0) + 1
                hit.add(ht)
            want_miss = np.array([miss.get(v, 0) for v in vox])
            want_hit = np.array([v in hit for v in vox])
            assert np.array_equal(got["misses"], want_miss) and np.array_equal(got["hit"], want_hit)
            remove = (want_miss >= min_misses) & ~want_hit & ((count < protect) if protect else True)
            assert np.array_equal(got["keep"], ~remove) and 0 < remove.sum() < len(vox)
            assert got["n_rays"] == len(pts) and got["n_rays_skipped"] == 4
            assert got["n_steps"] == steps and got["n_removed"] == remove.sum()
            assert got["n_points_removed"] == count[remove].sum()
            assert got["n_voxels_crossed"] == (want_miss > 0).sum() and got["n_voxels_hit"] == want_hit.sum()
    # the edge of the coordinate range: voxels 2^20 - 1 and -(2^20 - 1) are the last a ray may end in
    edge = np.float32([[524287.75, 0.0, 0.0], [524288.0, 0.0, 0.0], [0.0, -524287.5, 0.0], [0.0, -524287.75, 0.0]])
    got = carve_numpy(np.zeros((0, 3)), np.zeros(0), edge, [0.25, 0.25, 0.25], leaf, max_steps=5)
    assert got["n_rays_skipped"] == 2 and got["n_steps"] == 10
    # an origin beyond the range: every ray is skipped
    got = carve_numpy(np.zeros((0, 3)), np.zeros(0), edge, [524288.0, 0.0, 0.0], leaf)
    assert got["n_rays_skipped"] == 4 and got["n_steps"] == 0


def test_every_voxel_of_a_path_touches_its_segment():
    """The walk is a voxel traversal of the segment gs -> ge: consecutive voxels share a face, the path has |ve - vs|_1
    steps, and every voxel's cube, widened by 1e-9 (the walk's own rounding: t values are O(1) in f64), meets the
    segment."""
    rng = np.random.default_rng(6)
    for _ in range(200):
        gs, ge = rng.uniform(-20, 20, 3), rng.uniform(-20, 20, 3)
        gs, ge = to_grid(np.float32(gs), 1.0), to_grid(np.float32(ge), 1.0)
        path = np.array(walk(gs, ge), np.float64)
        assert len(path) - 1 == int(np.abs(np.floor(ge) - np.floor(gs)).sum())
        assert (np.abs(np.diff(path, axis=0)).sum(axis=1) == 1).all()
        d = ge - gs
        lo, hi = path - 1e-9, path + 1 + 1e-9
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - gs) / d, (hi - gs) / d
        flat = d == 0
        tn = np.where(flat, -np.inf, np.minimum(t0, t1)).max(axis=1)
        tf = np.where(flat, np.inf, np.maximum(t0, t1)).min(axis=1)
        inside_flat = ((gs >= lo) & (gs <= hi))[:, flat].all(axis=1)
        assert (inside_flat & (np.maximum(tn, 0.0) <= np.minimum(tf, 1.0))).all()


# ---- the scene of the GPU tests ------------------------------------------------------------------------------------------
SCENE_LEAF = 0.5
SCENE_GROUND_Z, SCENE_WALL_X = -1.52, 12.0
SCENE_CAR = (np.array([5.0, -1.0, SCENE_GROUND_Z]), np.array([7.0, 1.0, -0.3]))


def carve_scene(cols=96, rows=32):
    """Three scans in the sensor's own frame, all from `origin`: a ground plane, a wall and -- in the first scan only -- a
    box-shaped car in front of the wall; the third looks through where the car was.  The scans differ by a fraction of
    the beam spacing, as three revolutions of one lidar do.  The ground lies 2 cm below a voxel boundary: a ray that comes
    down at 8.6 degrees or more (the ground ends at the wall) covers at most 13 cm inside the ground's voxel layer, so it
    crosses at most one ground voxel before the one it ends in -- what keep_last = 1 is for.
    Returns dict(origin, scans [3] of float32 [cols * rows, 3], kinds [3]: 1 ground, 2 wall, 3 car)."""
    origin = np.float32([0.1, -0.05, 0.3])
    az = np.deg2rad(np.linspace(-35, 35, cols))
    el = np.deg2rad(np.linspace(-25, 8, rows))

    def cast(with_car, jitter):
        A, E = np.meshgrid(az + jitter * (az[1] - az[0]), el + jitter * (el[1] - el[0]), indexing="ij")
        d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
        o = origin.astype(np.float64)
        with np.errstate(divide="ignore"):
            tg = (SCENE_GROUND_Z - o[2]) / d[:, 2]
            tg[tg <= 0] = np.inf
            tw = (SCENE_WALL_X - o[0]) / d[:, 0]
        t, kind = np.minimum(tg, tw), np.where(tg < tw, 1, 2)
        if with_car:
            with np.errstate(divide="ignore", invalid="ignore"):
                t0, t1 = (SCENE_CAR[0] - o) / d, (SCENE_CAR[1] - o) / d
            tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
            on_car = (tn <= tf) & (tn > 0) & (tn < t)
            t, kind = np.where(on_car, tn, t), np.where(on_car, 3, kind)
        return (o + t[:, None] * d).astype(np.float32), kind

    casts = [cast(True, 0.0), cast(False, 0.37), cast(False, 0.71)]
    return dict(origin=origin, scans=[c[0] for c in casts], kinds=[c[1] for c in casts])


def scene_voxels(scene, pose=None):
    """the voxel sets of the scene's map (the first two scans): car (voxels that hold car returns only), wall, ground"""
    from test_map_target_cpu import voxel_ijk
    moved = [s if pose is None else host_transform_f64(pose, s) for s in scene["scans"][:2]]

    def keys(parts):
        sel = [m[k] for m, k in parts if len(m[k])]
        return set(map(tuple, voxel_ijk(np.concatenate(sel), SCENE_LEAF))) if sel else set()

    kinds = scene["kinds"][:2]
    car = keys([(moved[0], kinds[0] == 3)])
    wall = keys([(m, k == 2) for m, k in zip(moved, kinds)])
    ground = keys([(m, k == 1) for m, k in zip(moved, kinds)])
    return car - wall - ground, wall, ground


def test_the_scene_carves_the_car_and_nothing_else():
    """On the CPU, with the restatement alone: under the default parameters the third scan removes every car voxel, no
    wall voxel and no ground voxel; without keep_last the grazing rays take ground voxels away as well."""
    from test_map_state_cpu import mapstate_numpy
    scene = carve_scene()
    st = mapstate_numpy(np.concatenate(scene["scans"][:2]), SCENE_LEAF)
    car, wall, ground = scene_voxels(scene)
    assert len(car) >= 10 and len(wall) >= 200 and len(ground) >= 200 and (scene["kinds"][0] == 3).sum() > 300
    want = carve_numpy(st["ijk"], st["count"], scene["scans"][2], scene["origin"], SCENE_LEAF, **DEFAULTS)
    removed = set(map(tuple, st["ijk"][~want["keep"]]))
    assert removed == car and want["n_removed"] == len(car)
    assert not (removed & wall) and not (removed & ground)
    graze = carve_numpy(st["ijk"], st["count"], scene["scans"][2], scene["origin"], SCENE_LEAF, **dict(DEFAULTS, keep_last=0))
    removed0 = set(map(tuple, st["ijk"][~graze["keep"]]))
    assert car <= removed0 and len(removed0 & ground) >= 10 and not (removed0 & wall)


# ---- the kernels --------------------------------------------------------------------------------------------------------
def test_map_carve_kernels_do_not_spill(tmp_path):
    path = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_map_carve.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", ln)
        if m and name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    assert usage and all("k_mapcarve_" in k for k in usage), sorted(usage)
    kernels = {re.search(r"k_mapcarve_[a-z]+", k).group(0) for k in usage}
    assert kernels == {"k_mapcarve_rays", "k_mapcarve_count", "k_mapcarve_move"}, kernels
    for k, u in usage.items():
        assert u["ScratchSize"] == 0, (k, u)
    src = open(path).read()
    assert len(re.findall(r"__global__ void __launch_bounds__\(", src)) == len(re.findall(r"__global__", src)) == len(kernels)
    # integer atomics only, no inline assembly
    assert not re.search(r"atomicAdd\([^;]*float|unsafeAtomicAdd|\basm\b|__asm", src)
    # the read-only probe sits beside the claiming one, and the new file is part of the library
    shared = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_map_device.h")).read()
    assert shared.index("map_slot_of(") < shared.index("map_find(")
    assert not re.search(r"atomic", shared[shared.index("long long map_find("):shared.index("struct MapSel")])   # read only
    assert '#include "ndt_map_device.h"' in src and "map_find(" in src
    assert "$(B)/ndt_map_carve.o" in open(os.path.join(ROOT, "slam-sam_amd", "csrc", "Makefile")).read()
