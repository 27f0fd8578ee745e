"""CPU checks of the map's re-pose (ndt_map_transform, ndt_map_import_state_posed / _device; no GPU): the three symbols are
declared with their parameter lists, exported, listed and bound; a NULL handle and a NULL pose are refused before the
handle is looked at, and the Python mirror refuses a missing, misshapen or non-finite pose and ragged arrays before the
library is called; the kernels of ndt_map_repose.hip compile for gfx950 without scratch.
The NumPy yardstick the GPU tests compare with lives here: `repose_records` is the per-record rule of include/ndt_hip.h
written elementwise (every operation one IEEE rounding, in the order the header gives), `merge_records` the import's merge
of records in input order, `repose_numpy` the two together.  Its own check: on a lattice scene, where every sum is exact,
it commutes with adding the moved points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_map_state_cpu import mapstate_numpy, state_key, states_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_map_transform", "ndt_map_import_state_posed", "ndt_map_import_state_posed_device")
LIMIT = 1 << 20


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def repose_records(state, pose, leaf):
    """Every record of `state` (dict ijk, count, sums [n, 4] f32, moments [n, 9] f64 or None) moved by the upper 3 x 4 of
    `pose` as the header's rule says; the records stay in input order and are NOT merged.  Returns (records, n_bad): ijk of
    a record whose moved centroid is not finite or leaves |ijk| < 2^20 is meaningless and the record is counted in n_bad."""
    P = np.asarray(pose, np.float64)
    R, t = P[:3, :3], P[:3, 3]
    count = np.asarray(state["count"], np.int32)
    n = count.astype(np.float64)
    s = np.asarray(state["sums"], np.float32)
    nt = [n * t[a] for a in range(3)]

    def lin(a, v0, v1, v2):
        return (R[a, 0] * v0 + R[a, 1] * v1) + R[a, 2] * v2

    sd = [s[:, k].astype(np.float64) for k in range(3)]
    sums = np.zeros((len(count), 4), np.float32)
    with np.errstate(all="ignore"):
        for a in range(3):
            sums[:, a] = (lin(a, *sd) + nt[a]).astype(np.float32)
        sums[:, 3] = s[:, 3]
        mom = None
        if state.get("moments") is not None:
            q = np.asarray(state["moments"], np.float64)
            u = [lin(a, q[:, 0], q[:, 1], q[:, 2]) for a in range(3)]
            M = [[q[:, 3], q[:, 4], q[:, 5]], [q[:, 4], q[:, 6], q[:, 7]], [q[:, 5], q[:, 7], q[:, 8]]]
            A = [[lin(a, M[0][b], M[1][b], M[2][b]) for b in range(3)] for a in range(3)]
            mom = np.zeros((len(count), 9), np.float64)
            w = 3
            for a in range(3):
                mom[:, a] = u[a] + nt[a]
                for b in range(a, 3):
                    B = (A[a][0] * R[b, 0] + A[a][1] * R[b, 1]) + A[a][2] * R[b, 2]
                    mom[:, w] = ((B + u[a] * t[b]) + t[a] * u[b]) + nt[a] * t[b]
                    w += 1
        c = sums[:, :3] / count.astype(np.float32)[:, None]                   # f32 division
        f = np.floor(c * (np.float32(1.0) / np.float32(leaf)))                # f32 product, the add's binning
    ok = np.isfinite(c).all(axis=1) & (np.abs(f) < LIMIT).all(axis=1)
    ijk = np.where(ok[:, None], f, 0).astype(np.int32)
    return dict(ijk=ijk, count=count.copy(), sums=sums, moments=mom), int((~ok).sum())


def merge_records(base, rec):
    """The records `rec` (in input order; several may name one voxel) merged into the state `base` (None: an empty map) by
    the import's rule: per voxel its records in input order, every field old + record with one rounding; a voxel new to
    the map starts from +0.  Ascending (k, j, i)."""
    with_mom = rec.get("moments") is not None and (base is None or base.get("moments") is not None)
    kr = state_key(rec["ijk"])
    kb = state_key(base["ijk"]) if base is not None else np.zeros(0, np.int64)
    keys = np.union1d(kb, kr)
    m = len(keys)
    ijk = np.zeros((m, 3), np.int32)
    count = np.zeros(m, np.int32)
    sums = np.zeros((m, 4), np.float32)
    mom = np.zeros((m, 9), np.float64) if with_mom else None
    if base is not None:
        ib = np.searchsorted(keys, kb)
        ijk[ib], count[ib], sums[ib] = base["ijk"], base["count"], base["sums"]
        if with_mom:
            mom[ib] = base["moments"]
    order = np.argsort(kr, kind="stable")
    ks = kr[order]
    heads = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0] if len(ks) else np.zeros(0, np.int64)
    runs = np.diff(np.r_[heads, len(ks)])
    at = np.searchsorted(keys, ks[heads])
    ijk[at] = np.asarray(rec["ijk"], np.int32)[order[heads]]
    for j in range(int(runs.max()) if len(runs) else 0):                     # the j-th record of every voxel per step
        live = runs > j
        src, dst = order[heads[live] + j], at[live]
        sums[dst] = sums[dst] + np.asarray(rec["sums"], np.float32)[src]
        count[dst] = count[dst] + np.asarray(rec["count"], np.int32)[src]
        if with_mom:
            mom[dst] = mom[dst] + rec["moments"][src]
    return dict(ijk=ijk, count=count, sums=sums, moments=mom)


def repose_numpy(state, pose, leaf, into=None):
    """What ndt_map_transform makes of `state` (into=None), or ndt_map_import_state_posed of the records `state` on a map
    that holds `into`.  Refuses, as the library does, when a record cannot be placed."""
    rec, bad = repose_records(state, pose, leaf)
    if bad:
        raise OverflowError("%d record(s) cannot be placed" % bad)
    return merge_records(into, rec)


def rigid_pose(yaw=0.3, roll=0.02, pitch=-0.015, t=(10.3, -4.7, 0.21)):
    """the general rigid pose of the GPU tests: Rz(yaw) Ry(pitch) Rx(roll) and a translation"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def affine(R, t):
    T = np.eye(4)
    T[:3, :3] = np.asarray(R, np.float64)
    T[:3, 3] = t
    return T


LATTICE_POSES = {
    "identity": affine(np.eye(3), (0.0, 0.0, 0.0)),
    "shift": affine(np.eye(3), (1.5, -2.0, 0.5)),
    "rz90": affine([[0, -1, 0], [1, 0, 0], [0, 0, 1]], (3.0, -1.5, 7.0)),
    "flip": affine(np.diag([1.0, -1.0, -1.0]), (0.5, 0.5, -4.0)),
    "cycle": affine([[0, 0, 1], [1, 0, 0], [0, 1, 0]], (-2.0, 2.5, 1.0)),
}


def lattice_scene(n_voxels=300, seed=5, leaf=0.5, max_per_voxel=40, extent=20):
    """Points on multiples of 1/64 strictly inside their voxels of edge 0.5 (31 inner positions per axis), up to 40 per
    voxel, |coordinates| < 32 also after the lattice poses above: every f32 and f64 sum of a voxel is exact, so the state
    depends on no order and a lattice symmetry moves it exactly.  Shuffled; float32 [n, 3]."""
    rng = np.random.default_rng(seed)
    side = int(2 * extent / leaf)
    cells = rng.choice(side ** 3, n_voxels, replace=False)
    vox = np.stack([cells % side, (cells // side) % side, cells // side ** 2], axis=1) - side // 2
    per = rng.integers(1, max_per_voxel + 1, n_voxels)
    per[:3] = (1, 2, max_per_voxel)
    base = np.repeat(vox, per, axis=0).astype(np.float64) * leaf
    inner = rng.integers(1, 32, (len(base), 3)).astype(np.float64) / 64.0
    pts = (base + inner).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64), base + inner)
    return pts[rng.permutation(len(pts))]


def move_points(T, pts):
    """R p + t in f64, exact for lattice poses on lattice points, as float32"""
    q = pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    out = q.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), q)
    return out


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    want = {
        "ndt_map_transform": [vp, dp, C.POINTER(C.c_int64)],
        "ndt_map_import_state_posed": [vp, C.c_float, vp, vp, vp, vp, C.c_size_t, dp],
        "ndt_map_import_state_posed_device": [vp, C.c_float, vp, vp, vp, vp, C.c_size_t, dp],
    }
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int ndt_map_transform(ndt_handle* h, const double pose16_colmajor[16], int64_t* n_voxels_after_or_null);" in flat
    imp = ("(ndt_handle* h, float leaf, const int32_t* ijk, const int32_t* count, const float* sums4, "
           "const double* moments9, size_t n, const double pose16_colmajor[16]);")
    assert "int ndt_map_import_state_posed" + imp in flat and "int ndt_map_import_state_posed_device" + imp in flat
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    hpp = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    for m in ("mapTransform", "mapImportStatePosed", "mapImportStatePosedDevice"):
        assert callable(getattr(pkg, m)), m
        assert re.search(r"\b%s\s*\(" % m, hpp), m
    mk = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "Makefile")).read()
    assert "$(B)/ndt_map_repose.o" in mk


def test_argument_errors_come_before_the_handle(pkg):
    L = pkg.lib()
    pose = (C.c_double * 16)(*np.eye(4).ravel())
    ijk = (C.c_int32 * 6)()
    cnt = (C.c_int32 * 2)()
    sums = (C.c_float * 8)()
    mom = (C.c_double * 18)()
    after = C.c_int64(7)
    # NULL handle
    assert L.ndt_map_transform(None, pose, C.byref(after)) == -1
    assert L.ndt_map_import_state_posed(None, 0.5, ijk, cnt, sums, mom, 2, pose) == -1
    assert L.ndt_map_import_state_posed_device(None, 0.5, None, None, None, None, 0, pose) == -1
    # the argument checks come before the handle is looked at: a stand-in block of zero bytes is never read
    h = C.create_string_buffer(1 << 16)
    assert L.ndt_map_transform(h, None, C.byref(after)) == -1                       # NULL pose
    for fn in (L.ndt_map_import_state_posed, L.ndt_map_import_state_posed_device):
        assert fn(h, 0.5, ijk, cnt, sums, mom, 2, None) == -1                       # NULL pose
        assert fn(h, 0.5, ijk, cnt, sums, mom, 0, None) == -1                       # ... also with nothing to import
        assert fn(h, 0.5, None, cnt, sums, mom, 2, pose) == -1
        assert fn(h, 0.5, ijk, None, sums, mom, 2, pose) == -1
        assert fn(h, 0.5, ijk, cnt, None, mom, 2, pose) == -1
    assert after.value == 7 and bytes(h.raw) == bytes(1 << 16)                      # nothing was written
    assert not any(ijk) and not any(cnt) and not any(sums) and not any(mom)


def test_python_mirror_validates_before_the_library(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)   # no handle: nothing may reach the library
    ndt._h = None
    eye = np.eye(4)
    nan = np.eye(4)
    nan[1, 3] = np.nan
    inf = np.eye(4)
    inf[3, 0] = np.inf
    ok = dict(leaf=0.5, ijk=np.zeros((2, 3)), count=np.ones(2), sums=np.zeros((2, 4)), moments=None)
    bad = [
        lambda: pkg.mapTransform(ndt, None), lambda: pkg.mapTransform(ndt, np.eye(3)), lambda: pkg.mapTransform(ndt, np.zeros(16)),
        lambda: pkg.mapTransform(ndt, nan), lambda: pkg.mapTransform(ndt, inf),
        lambda: pkg.mapImportStatePosed(ndt, ok), lambda: pkg.mapImportStatePosed(ndt, ok, None), lambda: pkg.mapImportStatePosed(ndt, ok, nan),
        lambda: pkg.mapImportStatePosed(ndt, ok, np.eye(3)),
        lambda: pkg.mapImportStatePosed(ndt, dict(ok, count=np.ones(3)), eye),
        lambda: pkg.mapImportStatePosed(ndt, dict(ok, sums=np.zeros((2, 3))), eye),
        lambda: pkg.mapImportStatePosed(ndt, dict(ok, moments=np.zeros((1, 9))), eye),
        lambda: pkg.mapImportStatePosed(ndt, pose=eye, ijk=np.zeros((2, 3)), count=np.ones(2), sums=np.zeros((2, 4))),      # no leaf
        lambda: pkg.mapImportStatePosedDevice(ndt, 0.5, 1, 2, 3, None, 2, None),
        lambda: pkg.mapImportStatePosedDevice(ndt, 0.5, 1, 2, 3, None, 2, inf),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d reached the library" % k)


# ---- the yardstick's own check ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice():
    pts = lattice_scene()
    return pts, mapstate_numpy(pts, 0.5)


@pytest.mark.parametrize("name", sorted(LATTICE_POSES))
def test_the_rule_commutes_with_adding_points_under_lattice_symmetries(lattice, name):
    pts, st = lattice
    T = LATTICE_POSES[name]
    assert len(st["count"]) == 300 and st["count"].max() == 40 and np.abs(pts).max() < 32
    got = repose_numpy(st, T, 0.5)
    want = mapstate_numpy(move_points(T, pts), 0.5)
    assert len(want["count"]) == 300                                            # a symmetry merges nothing
    assert states_equal(got, want), name
    if name == "identity":
        assert states_equal(got, st)
    no_mom = repose_numpy(dict(st, moments=None), T, 0.5)                       # the float centroid decides, moments or not
    assert no_mom["moments"] is None and states_equal(no_mom, want, moments=False)


def test_invariants_under_a_general_rigid_pose():
    rng = np.random.default_rng(3)
    pts = rng.uniform([-40, -30, -2], [40, 30, 6], (20000, 3)).astype(np.float32)
    st = mapstate_numpy(pts, 1.0)
    T = rigid_pose()
    rec, bad = repose_records(st, T, 1.0)
    assert bad == 0
    out = merge_records(None, rec)
    assert out["count"].sum() == st["count"].sum() == len(pts)                  # no point is lost
    assert len(out["count"]) <= len(st["count"])
    assert np.array_equal(state_key(out["ijk"]), np.sort(state_key(out["ijk"])))
    # sum m1' = R sum m1 + N t: each record adds a few roundings at the size of its largest term, n |x| <= count * 60
    R, t, N = T[:3, :3], T[:3, 3], float(len(pts))
    want = R @ st["moments"][:, :3].sum(axis=0) + N * t
    scale = (st["count"] * 60.0).sum()
    assert np.abs(out["moments"][:, :3].sum(axis=0) - want).max() <= 8 * np.finfo(np.float64).eps * scale
    # the second moments stay symmetric positive semi-definite about the mean for every voxel with 3+ points
    big = out["count"] >= 3
    n = out["count"][big].astype(np.float64)
    m1, q = out["moments"][big, :3], out["moments"][big, 3:]
    var = np.stack([q[:, 0], q[:, 3], q[:, 5]], axis=1) - m1 * m1 / n[:, None]
    assert (var > -1e-6 * n[:, None]).all()
    # a record that cannot be placed is counted, and repose_numpy refuses
    far = affine(np.eye(3), (2.0 ** 21, 0.0, 0.0))
    assert repose_records(st, far, 1.0)[1] == len(st["count"])
    with pytest.raises(OverflowError):
        repose_numpy(st, far, 1.0)


def test_merge_records_applies_repeated_voxels_in_input_order():
    rec = dict(ijk=np.array([[1, 2, 3], [0, 0, 0], [1, 2, 3], [1, 2, 3]], np.int32), count=np.array([1, 2, 3, 4], np.int32),
               sums=np.array([[1e8, 0, 0, 0], [1, 1, 1, 1], [1, 0, 0, 0], [-1e8, 0, 0, 0]], np.float32),
               moments=np.zeros((4, 9)))
    rec["moments"][:, 0] = [1e17, 1.0, 1.0, -1e17]
    out = merge_records(None, rec)
    assert np.array_equal(out["ijk"], [[0, 0, 0], [1, 2, 3]]) and np.array_equal(out["count"], [2, 8])
    assert out["sums"][1, 0] == np.float32(np.float32(np.float32(1e8) + np.float32(1)) - np.float32(1e8)) == 0.0
    assert out["moments"][1, 0] == (1e17 + 1.0) - 1e17 == 0.0                   # ((0 + a) + b) + c, not a + (b + c)
    base = dict(ijk=np.array([[1, 2, 3]], np.int32), count=np.array([5], np.int32), sums=np.ones((1, 4), np.float32),
                moments=np.ones((1, 9)))
    out = merge_records(base, rec)
    assert np.array_equal(out["count"], [2, 13]) and out["sums"][1, 1] == 1.0 and out["moments"][1, 1] == 1.0


# ---- the kernels --------------------------------------------------------------------------------------------------------
def test_map_repose_kernels_do_not_spill(tmp_path):
    """The figures tools/kernel_resources.py prints for `ndt_map_repose.hip k_maprepose_`: every kernel without scratch."""
    path = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_map_repose.hip")
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
    assert usage and all("k_maprepose_" in k for k in usage), sorted(usage)          # the new kernels carry the prefix
    kernels = {re.search(r"k_maprepose_[a-z]+", k).group(0) for k in usage}
    assert kernels == {"k_maprepose_records"}, kernels
    assert len(usage) == 2                                                            # with and without moments
    for k, u in usage.items():
        assert u["ScratchSize"] == 0, (k, u)
    src = open(path).read()
    assert len(re.findall(r"__global__ void __launch_bounds__\(", src)) == len(re.findall(r"__global__", src)) == len(kernels)
    # integer atomics only (those of the shared statistics helper), no inline assembly, and the import's tail is called,
    # not copied: no sort, run search or accumulate launch of its own
    assert not re.search(r"atomic\w*\(|\basm\b", src)
    assert "map_import_tail(" in src and "map_merge_records(" in src and "map_record_stats(" in src
    assert not re.search(r"sort_keyed\(|sort_pairs\(|find_runs\(|hipLaunchKernelGGL\(k_(?!maprepose_)", src)
    # ndt_map_state.hip gained no kernel (its own test pins the set) and shares the statistics helper
    state = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_map_state.hip")).read()
    assert "map_record_stats(" in state
