"""CPU checks of the map-state boundary (ndt_map_crop, ndt_map_export_state / _device, ndt_map_import_state / _device; no
GPU): the five symbols are declared with their parameter lists, exported, listed and bound; bad arguments are refused
before the handle is looked at, and the Python mirror refuses half a box, a non-finite box and ragged arrays before the
library is called; the kernels of ndt_map_state.hip compile for gfx950 without scratch.
The NumPy yardsticks the GPU tests compare with live here: `mapstate_numpy` (per voxel ijk, count, sequential f32 sums and
sequential f64 moments, ascending (k, j, i)) and `continue_numpy` (the same, going on from a given state) -- checked
against the two yardsticks the project already trusts, of which they are the un-divided form -- and `merge_numpy` (old +
record per field, one rounding)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_voxel_map import voxelmap_numpy
from test_map_target_cpu import host_transform_f64, moments_numpy, voxel_ijk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_map_crop", "ndt_map_export_state", "ndt_map_export_state_device", "ndt_map_import_state",
       "ndt_map_import_state_device")


# ---- yardsticks ---------------------------------------------------------------------------------------------------------
def state_key(ijk):
    """the map's 63-bit voxel key: ascending keys are ascending (k, j, i)"""
    v = np.asarray(ijk, np.int64).reshape(-1, 3) + (1 << 20)
    return (v[:, 2] << 42) | (v[:, 1] << 21) | v[:, 0]


def continue_numpy(st, pts, leaf, intensity=None):
    """The state `st` (None: an empty map) after `pts` were added: every voxel's f32 sums and f64 moments go on from what
    `st` holds, one point at a time in input order (vectorised over the voxels, one point of every voxel per step); a
    voxel new to the state starts from zero.  Non-finite points are skipped.  Ascending (k, j, i)."""
    p = np.asarray(pts, np.float32)[:, :3]
    fin = np.isfinite(p).all(axis=1)
    q = p[fin]
    ijk = voxel_ijk(q, leaf)
    order = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))          # stable; the last key is the primary one
    s = ijk[order]
    heads = np.nonzero(np.r_[True, (s[1:] != s[:-1]).any(axis=1)])[0] if len(s) else np.zeros(0, np.int64)
    counts = np.diff(np.r_[heads, len(s)])
    f = np.zeros((len(q), 4), np.float32)
    f[:, :3] = q[order]
    if intensity is not None:
        f[:, 3] = np.asarray(intensity, np.float32)[fin][order]
    d = q[order].astype(np.float64)
    a, b, c = d[:, 0], d[:, 1], d[:, 2]
    g = np.stack([a, b, c, a * a, a * b, a * c, b * b, b * c, c * c], axis=1)   # products of f32 values: exact in f64
    knew = state_key(s[heads])
    kold = state_key(st["ijk"]) if st is not None else np.zeros(0, np.int64)
    keys = np.union1d(kold, knew)
    io, at_new = np.searchsorted(keys, kold), np.searchsorted(keys, knew)
    m = len(keys)
    out_ijk = np.zeros((m, 3), np.int32)
    out_ijk[at_new] = s[heads]
    total = np.zeros(m, np.int32)
    total[at_new] = counts
    sums = np.zeros((m, 4), np.float32)
    mom = np.zeros((m, 9), np.float64)
    if st is not None:
        out_ijk[io] = st["ijk"]
        total[io] = total[io] + st["count"]
        sums[io] = st["sums"]
        mom[io] = st["moments"]
    for j in range(int(counts.max()) if len(counts) else 0):
        live = counts > j
        src, dst = heads[live] + j, at_new[live]
        sums[dst] = sums[dst] + f[src]
        mom[dst] = mom[dst] + g[src]
    return dict(ijk=out_ijk, count=total, sums=sums, moments=mom)


def mapstate_numpy(pts, leaf, intensity=None):
    """dict(ijk [m,3] int32, count [m] int32, sums [m,4] f32 = sum x, y, z, intensity (0 without), moments [m,9] f64) of the
    occupied voxels in ascending (k, j, i) order; non-finite points skipped; every sum sequential in input order: what a
    map fed `pts` in any split holds."""
    return continue_numpy(None, pts, leaf, intensity)


def filter_state(st, keep):
    return dict(ijk=st["ijk"][keep], count=st["count"][keep], sums=st["sums"][keep],
                moments=None if st.get("moments") is None else st["moments"][keep])


def merge_numpy(a, b):
    """State `b` (one record per voxel) imported into state `a`: per field old + record in f32 / f64, one rounding; a voxel
    only `b` has starts from +0; a voxel only `a` has is untouched.  Ascending (k, j, i)."""
    ka, kb = state_key(a["ijk"]), state_key(b["ijk"])
    assert len(np.unique(ka)) == len(ka) and len(np.unique(kb)) == len(kb)
    keys = np.union1d(ka, kb)
    ia, ib = np.searchsorted(keys, ka), np.searchsorted(keys, kb)
    m = len(keys)
    ijk = np.zeros((m, 3), np.int32)
    ijk[ia] = a["ijk"]
    ijk[ib] = b["ijk"]
    count = np.zeros(m, np.int32)
    count[ia] = a["count"]
    count[ib] = count[ib] + b["count"]
    sums = np.zeros((m, 4), np.float32)
    sums[ia] = a["sums"]
    sums[ib] = sums[ib] + np.asarray(b["sums"], np.float32)
    mom = None
    if a.get("moments") is not None and b.get("moments") is not None:
        mom = np.zeros((m, 9), np.float64)
        mom[ia] = a["moments"]
        mom[ib] = mom[ib] + b["moments"]
    return dict(ijk=ijk, count=count, sums=sums, moments=mom)


def states_equal(a, b, moments=True):
    """bit for bit"""
    ok = (np.array_equal(a["ijk"], b["ijk"]) and np.array_equal(a["count"], b["count"]) and
          a["sums"].shape == b["sums"].shape and
          np.array_equal(np.ascontiguousarray(a["sums"], np.float32).view(np.uint32),
                         np.ascontiguousarray(b["sums"], np.float32).view(np.uint32)))
    if moments:
        ok = ok and a["moments"].shape == b["moments"].shape and np.array_equal(
            np.ascontiguousarray(a["moments"], np.float64).view(np.uint64),
            np.ascontiguousarray(b["moments"], np.float64).view(np.uint64))
    return bool(ok)


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    want = {
        "ndt_map_crop": [vp, fp, fp, C.c_int, C.POINTER(C.c_int64)],
        "ndt_map_export_state": [vp, fp, fp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)],
        "ndt_map_export_state_device": [vp, fp, fp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)],
        "ndt_map_import_state": [vp, C.c_float, vp, vp, vp, vp, C.c_size_t],
        "ndt_map_import_state_device": [vp, C.c_float, vp, vp, vp, vp, C.c_size_t],
    }
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int ndt_map_crop(ndt_handle* h, const float box_min[3], const float box_max[3], int remove_inside, "
            "int64_t* n_removed);") in flat
    exp = ("(ndt_handle* h, const float box_min[3], const float box_max[3], int32_t* ijk, int32_t* count, float* sums4, "
           "double* moments9, size_t cap, size_t* n_out);")
    imp = ("(ndt_handle* h, float leaf, const int32_t* ijk, const int32_t* count, const float* sums4, "
           "const double* moments9, size_t n);")
    assert "int ndt_map_export_state" + exp in flat and "int ndt_map_export_state_device" + exp in flat
    assert "int ndt_map_import_state" + imp in flat and "int ndt_map_import_state_device" + imp in flat
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    assert C.sizeof(pkg.MapInfo) == 80
    hpp = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    for m in ("mapCrop", "mapExportState", "mapImportState"):
        assert callable(getattr(pkg.NormalDistributionsTransform, m)), m
        assert re.search(r"\b%s\s*\(" % m, hpp), m


def test_argument_errors_come_before_the_handle(pkg):
    L = pkg.lib()
    box = (C.c_float * 3)(0.0, 0.0, 0.0)
    ijk = (C.c_int32 * 6)()
    cnt = (C.c_int32 * 2)()
    sums = (C.c_float * 8)()
    mom = (C.c_double * 18)()
    removed = C.c_int64(7)
    m = C.c_size_t(7)
    # NULL handle
    assert L.ndt_map_crop(None, box, box, 0, C.byref(removed)) == -1
    assert L.ndt_map_export_state(None, None, None, ijk, cnt, sums, mom, 2, C.byref(m)) == -1
    assert L.ndt_map_export_state_device(None, None, None, None, None, None, None, 0, C.byref(m)) == -1
    assert L.ndt_map_import_state(None, 0.5, ijk, cnt, sums, mom, 2) == -1
    assert L.ndt_map_import_state_device(None, 0.5, None, None, None, None, 0) == -1
    # the argument checks come before the handle is looked at: a stand-in block of zero bytes is never read
    h = C.create_string_buffer(1 << 16)
    assert L.ndt_map_crop(h, None, box, 0, C.byref(removed)) == -1
    assert L.ndt_map_crop(h, box, None, 1, C.byref(removed)) == -1
    assert L.ndt_map_crop(h, None, None, 0, None) == -1
    for fn in (L.ndt_map_export_state, L.ndt_map_export_state_device):
        assert fn(h, box, None, ijk, cnt, sums, mom, 2, C.byref(m)) == -1          # half a box
        assert fn(h, None, box, ijk, cnt, sums, mom, 2, C.byref(m)) == -1
        assert fn(h, None, None, ijk, cnt, sums, mom, 2, None) == -1               # nowhere to put the size
    for fn in (L.ndt_map_import_state, L.ndt_map_import_state_device):
        assert fn(h, 0.5, None, cnt, sums, mom, 2) == -1
        assert fn(h, 0.5, ijk, None, sums, mom, 2) == -1
        assert fn(h, 0.5, ijk, cnt, None, mom, 2) == -1
    assert removed.value == 7 and m.value == 7 and bytes(h.raw) == bytes(1 << 16)    # nothing was written
    assert not any(ijk) and not any(cnt) and not any(sums) and not any(mom)


def test_python_mirror_validates_before_the_library(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)   # no handle: nothing may reach the library
    ndt._h = None
    lo, hi = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    bad = [
        lambda: ndt.mapCrop(lo, None), lambda: ndt.mapCrop(None, hi), lambda: ndt.mapCrop(None, None),
        lambda: ndt.mapCrop(lo, [1.0, np.nan, 1.0]), lambda: ndt.mapCrop([0.0, -np.inf, 0.0], hi), lambda: ndt.mapCrop([0, 0], hi),
        lambda: ndt.mapExportState(box_min=lo), lambda: ndt.mapExportState(box_max=hi),
        lambda: ndt.mapExportState(lo, [np.inf, 1.0, 1.0]),
        lambda: ndt.mapExportStateDevice(None, None, None, None, 0, box_min=lo),
        lambda: ndt.mapImportState(leaf=0.5, ijk=np.zeros((3, 3)), count=np.ones(2), sums=np.zeros((2, 4))),
        lambda: ndt.mapImportState(leaf=0.5, ijk=np.zeros((2, 3)), count=np.ones(2), sums=np.zeros((2, 3))),
        lambda: ndt.mapImportState(leaf=0.5, ijk=np.zeros((2, 3)), count=np.ones(2), sums=np.zeros((3, 4))),
        lambda: ndt.mapImportState(leaf=0.5, ijk=np.zeros((2, 3)), count=np.ones(2), sums=np.zeros((2, 4)), moments=np.zeros((1, 9))),
        lambda: ndt.mapImportState(dict(leaf=0.5, ijk=np.zeros((2, 3)), count=np.ones(3), sums=np.zeros((2, 4)), moments=None)),
        lambda: ndt.mapImportState(ijk=np.zeros((2, 3)), count=np.ones(2), sums=np.zeros((2, 4))),       # no leaf
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d reached the library" % k)


# ---- the yardsticks against the ones the project trusts ---------------------------------------------------------------
def test_the_state_yardstick_is_the_undivided_form_of_the_trusted_ones(pkg):
    from slam_sam_amd import replay
    stream = replay.make_stream(n_frames=4, beams=32, cols=256)
    base = np.concatenate([host_transform_f64(T, scan) for scan, T in stream])
    rng = np.random.default_rng(1)
    cloud = rng.uniform([-3, -2, -1], [3, 2, 1], (3000, 3)).astype(np.float32)
    cloud[::97] = np.nan
    cloud[5] = [-0.0, 0.5, -0.5]
    inten = rng.uniform(0, 255, 3000).astype(np.float32)
    for pts, leaf, it in ((base, 1.0, None), (base, 0.5, None), (cloud, 0.5, inten), (cloud, 0.3, None)):
        st = mapstate_numpy(pts, leaf, it)
        xyz, xi, counts, ijk = voxelmap_numpy(pts, leaf, it)
        assert np.array_equal(st["ijk"], ijk) and st["ijk"].dtype == np.int32 and np.array_equal(st["count"], counts)
        nf = st["count"].astype(np.float32)
        assert np.array_equal((st["sums"][:, :3] / nf[:, None]).view(np.uint32), xyz.view(np.uint32))     # as bits
        if it is not None:
            assert np.array_equal((st["sums"][:, 3] / nf).view(np.uint32), xi.view(np.uint32))
        else:
            assert not st["sums"][:, 3].any()
        mijk, mcount, msums = moments_numpy(pts, leaf)
        assert np.array_equal(st["ijk"], mijk) and np.array_equal(st["count"], mcount)
        assert np.array_equal(st["moments"], msums)
        assert np.array_equal(state_key(st["ijk"]), np.sort(state_key(st["ijk"])))            # ascending (k, j, i)
        assert not np.signbit(st["sums"][st["sums"] == 0]).any()                              # a map never holds -0.0
    # merge_numpy: a split at a point boundary, the two halves merged -- voxels one side alone has arrive bit for bit,
    # shared voxels are old + record with one rounding per field, counts and the voxel set are those of the whole
    a, b, whole = mapstate_numpy(base[:16384], 1.0), mapstate_numpy(base[16384:], 1.0), mapstate_numpy(base, 1.0)
    mg = merge_numpy(a, b)
    assert np.array_equal(mg["ijk"], whole["ijk"]) and np.array_equal(mg["count"], whole["count"])
    ka, kb, km = state_key(a["ijk"]), state_key(b["ijk"]), state_key(mg["ijk"])
    only_a, only_b = ~np.isin(km, kb), ~np.isin(km, ka)
    both = ~only_a & ~only_b
    assert only_a.sum() > 100 and only_b.sum() > 100 and both.sum() > 100
    assert states_equal(filter_state(mg, only_a), filter_state(a, ~np.isin(ka, kb)))
    assert states_equal(filter_state(mg, only_b), filter_state(b, ~np.isin(kb, ka)))
    sa, sb = filter_state(a, np.isin(ka, kb)), filter_state(b, np.isin(kb, ka))
    assert np.array_equal(mg["sums"][both], sa["sums"] + sb["sums"]) and np.array_equal(mg["moments"][both], sa["moments"] + sb["moments"])
    # (not bits: one more rounding.  |x| < 100 m and at most 179 points per voxel: partial sums below 1.8e6, whose f64
    # spacing is 2.3e-10)
    np.testing.assert_allclose(mg["moments"], whole["moments"], rtol=1e-12, atol=1e-9)
    # continue_numpy: a state continued with more points is the state of all the points, however they were split
    assert states_equal(continue_numpy(a, base[16384:], 1.0), whole)
    assert states_equal(continue_numpy(continue_numpy(None, base[:5], 1.0), base[5:], 1.0), whole)


# ---- the kernels --------------------------------------------------------------------------------------------------------
def test_map_state_kernels_do_not_spill(tmp_path):
    """The figures tools/kernel_resources.py prints for `ndt_map_state.hip k_mapstate_`: every kernel without scratch."""
    path = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_map_state.hip")
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
    assert usage and all("k_mapstate_" in k for k in usage), sorted(usage)           # the new kernels carry the prefix
    kernels = {re.search(r"k_mapstate_[a-z]+", k).group(0) for k in usage}
    assert kernels == {"k_mapstate_crop", "k_mapstate_gather", "k_mapstate_keys", "k_mapstate_accumulate"}, kernels
    assert len(usage) == 5                                                            # accumulate with and without moments
    for k, u in usage.items():
        assert u["ScratchSize"] == 0, (k, u)
    src = open(path).read()
    assert len(re.findall(r"__global__ void __launch_bounds__\(", src)) == len(re.findall(r"__global__", src)) == len(kernels)
    # integer atomics only, no inline assembly
    assert not re.search(r"atomicAdd\([^;]*float|unsafeAtomicAdd|\basm\b", src)
    # the helpers both translation units share moved to one header, and the map's own file includes it
    shared = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_map_device.h")).read()
    for name in ("MAP_EMPTY", "MAP_BIAS", "map_hash", "map_slot_of", "struct MapSel", "map_in_box", "wave_sum", "wave_min", "wave_max"):
        assert re.search(r"\b%s\b" % name, shared), name
    for f in ("ndt_map.hip", "ndt_map_state.hip"):
        assert '#include "ndt_map_device.h"' in open(os.path.join(ROOT, "slam-sam_amd", "csrc", f)).read()
