"""CPU checks of the connected-components boundary (ndt_map_components_default_params,
ndt_map_component_filter_default_params, ndt_map_components, ndt_map_export_components, ndt_map_export_labels / _device,
ndt_map_label_points / _device, ndt_map_remove_components; no GPU): the nine symbols are declared with their parameter
lists, exported, listed and bound, the five structs have their sizes and the defaults are 26, 1 and 1, 0, 0, 0, 0; NULL
and out-of-range arguments are refused before the handle is looked at, and the Python mirror refuses them before the
library; the kernels of ndt_map_components.hip compile for gfx950 without scratch.
The yardsticks the GPU tests compare with live here: `components_numpy`, rules 1-6 of the header comment restated as a
breadth-first search over a dict of voxels, and `remove_numpy`, the survive rule with ndt_map_crop's bookkeeping on a
state export.  Both work on integers only.  They are checked against hand-worked cases and, where scipy imports, against
scipy.ndimage.label on a dense box under the three structuring elements."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_map_state_cpu import state_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_map_components_default_params", "ndt_map_component_filter_default_params", "ndt_map_components",
       "ndt_map_export_components", "ndt_map_export_labels", "ndt_map_export_labels_device", "ndt_map_label_points",
       "ndt_map_label_points_device", "ndt_map_remove_components")
LIMIT = 1 << 20
CONNECTIVITIES = (6, 18, 26)
INFO_FIELDS = ("n_components", "n_voxels_labelled", "n_voxels_unlabelled", "largest", "largest_n_voxels", "largest_n_points")
REMOVE_FIELDS = ("n_components", "n_components_removed", "n_removed", "n_points_removed")
COMP_FIELDS = ("root_ijk", "n_voxels", "n_points", "min_ijk", "max_ijk")


# ---- the yardsticks -----------------------------------------------------------------------------------------------------
def offsets_of(connectivity):
    """rule 2: the offsets with every |d| <= 1 and 1 <= sum |d| <= 1, 2 or 3"""
    top = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(di, dj, dk) for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1)
            if 1 <= abs(di) + abs(dj) + abs(dk) <= top]


def components_numpy(ijk, count, connectivity=26, min_count=1):
    """Rules 1-6 on the voxels `ijk` [m, 3] with `count` [m] points, given in any order.  Returns a dict: `ijk` and
    `count` in ascending (k, j, i) order (ndt_map_export_state's), `label` [m] int32 in that order, `comps` (root_ijk
    [C, 3], n_voxels [C], n_points [C] int64, min_ijk / max_ijk [C, 3]) in index order and `info` (every field of
    ndt_map_components_info)."""
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    count = np.asarray(count, np.int64).reshape(-1)
    assert len(ijk) == len(count) and (np.abs(ijk) < LIMIT).all()
    order = np.argsort(state_key(ijk), kind="stable")
    ijk, count = ijk[order], count[order]
    assert len(np.unique(state_key(ijk))) == len(ijk)
    at = {tuple(v): r for r, v in enumerate(ijk.tolist())}
    eligible = count >= min_count                                          # rule 1
    label = np.full(len(ijk), -1, np.int32)
    offs = offsets_of(connectivity)
    roots = []
    for r in range(len(ijk)):                                              # ascending (k, j, i): rules 4 and 5
        if not eligible[r] or label[r] >= 0:
            continue
        c = len(roots)
        roots.append(r)                                                    # the first voxel of its component in this order
        label[r] = c
        todo = [r]
        while todo:
            i, j, k = ijk[todo.pop()].tolist()
            for di, dj, dk in offs:
                n = (i + di, j + dj, k + dk)
                if max(abs(n[0]), abs(n[1]), abs(n[2])) >= LIMIT:          # rule 3: no such neighbour
                    continue
                q = at.get(n)
                if q is not None and eligible[q] and label[q] < 0:
                    label[q] = c
                    todo.append(q)
    C_ = len(roots)
    comps = dict(root_ijk=ijk[roots].astype(np.int32).reshape(C_, 3), n_voxels=np.zeros(C_, np.int32), n_points=np.zeros(C_, np.int64),
                 min_ijk=np.zeros((C_, 3), np.int32), max_ijk=np.zeros((C_, 3), np.int32))
    for c in range(C_):
        sel = label == c
        comps["n_voxels"][c] = sel.sum()
        comps["n_points"][c] = count[sel].sum()
        comps["min_ijk"][c] = ijk[sel].min(0)
        comps["max_ijk"][c] = ijk[sel].max(0)
    big = int(np.argmax(comps["n_voxels"])) if C_ else -1                   # (argmax: the first of the largest)
    info = dict(n_components=C_, n_voxels_labelled=int(eligible.sum()), n_voxels_unlabelled=int((~eligible).sum()), largest=big,
                largest_n_voxels=int(comps["n_voxels"][big]) if C_ else 0, largest_n_points=int(comps["n_points"][big]) if C_ else 0)
    return dict(ijk=ijk.astype(np.int32), count=count.astype(np.int32), label=label, comps=comps, info=info)


def survivors_numpy(comps, min_voxels=1, min_points=0, keep_largest=0):
    """the survive rule: bool [C]"""
    nv, npts = np.asarray(comps["n_voxels"], np.int64), np.asarray(comps["n_points"], np.int64)
    ok = (nv >= min_voxels) & (npts >= min_points)
    if keep_largest > 0:
        rank = np.argsort(-nv, kind="stable")                              # n_voxels descending, index ascending
        among = np.zeros(len(nv), bool)
        among[rank[:keep_largest]] = True
        ok &= among
    return ok


def pow2_at_least(v):
    c = 64
    while c < v:
        c <<= 1
    return c


def remove_numpy(cc, info0, min_voxels=1, min_points=0, keep_largest=0, remove_unlabelled=False, dry_run=False):
    """ndt_map_remove_components on the labelling `cc` (components_numpy) of a map whose ndt_map_get_info is `info0`:
    dict(result: every field of ndt_map_remove_components_result, keep: bool per voxel of cc["ijk"], info: what
    ndt_map_get_info reports afterwards -- crop's bookkeeping)."""
    ok = survivors_numpy(cc["comps"], min_voxels, min_points, keep_largest)
    label = cc["label"]
    keep = np.where(label >= 0, ok[np.maximum(label, 0)] if len(ok) else False, not remove_unlabelled)
    keep = np.asarray(keep, bool).reshape(len(label))
    result = dict(n_components=len(ok), n_components_removed=int((~ok).sum()), n_removed=int((~keep).sum()),
                  n_points_removed=int(cc["count"][~keep].astype(np.int64).sum()))
    info = dict(info0)
    if not dry_run and result["n_removed"] > 0:
        kept = int(keep.sum())
        info["n_voxels"] = kept
        info["n_points"] = int(cc["count"][keep].astype(np.int64).sum())
        info["capacity"] = max(pow2_at_least(2 * kept), info0["reset_capacity"]) if "reset_capacity" in info0 else None
        if kept:
            info["min_ijk"] = tuple(int(v) for v in cc["ijk"][keep].min(0))
            info["max_ijk"] = tuple(int(v) for v in cc["ijk"][keep].max(0))
    if dry_run:
        keep = np.ones(len(label), bool)
    return dict(result=result, keep=keep, info=info)


def map_hash_numpy(keys):
    """map_hash of ndt_map_device.h (splitmix64's finaliser) on uint64 keys"""
    k = np.asarray(keys, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(30)
        k *= np.uint64(0xbf58476d1ce4e5b9)
        k ^= k >> np.uint64(27)
        k *= np.uint64(0x94d049bb133111eb)
        k ^= k >> np.uint64(31)
    return k


def snake_voxels(n=16):
    """a one-voxel-wide serpentine through every voxel of an n^3 box: consecutive voxels share a face, no others do ...
    in the plane; the planes are joined at one end only -- so it is NOT used as it is: see snake_path"""
    out = []
    for k in range(n):
        plane = []
        for j in range(n):
            row = [(i, j, k) for i in range(n)]
            plane += row if j % 2 == 0 else row[::-1]
        out += plane if k % 2 == 0 else plane[::-1]
    return np.array(out, np.int64)


def snake_path(length=4096):
    """A one-voxel-wide path of `length` voxels whose ONLY face adjacencies are those of consecutive voxels: a serpentine
    on the lattice of spacing 2 (rows along i, joined at alternating ends, planes joined likewise), every lattice step
    made of two voxels.  Under connectivity 6 it is one component whose diameter is its length; without one voxel of its
    middle it is two."""
    cells = snake_voxels(16)                                               # 4096 lattice cells, consecutive ones adjacent
    out = []
    for a, b in zip(cells[:-1], cells[1:]):
        out.append(2 * a)
        out.append(a + b)                                                  # the voxel between two lattice cells
    out.append(2 * cells[-1])
    return np.array(out[:length], np.int64)


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, dp, sz = C.c_void_p, C.POINTER(C.c_double), C.c_size_t
    pp, fp_ = C.POINTER(pkg.MapComponentsParams), C.POINTER(pkg.MapComponentFilter)
    szp, i64p = C.POINTER(C.c_size_t), C.POINTER(C.c_int64)
    want = {
        "ndt_map_components_default_params": [pp],
        "ndt_map_component_filter_default_params": [fp_],
        "ndt_map_components": [vp, pp, C.POINTER(pkg.MapComponentsInfo)],
        "ndt_map_export_components": [vp, pp, C.POINTER(pkg.MapComponent), sz, szp],
        "ndt_map_export_labels": [vp, pp, vp, vp, sz, szp],
        "ndt_map_export_labels_device": [vp, pp, vp, vp, sz, szp],
        "ndt_map_label_points": [vp, pp, vp, sz, sz, dp, vp, i64p],
        "ndt_map_label_points_device": [vp, pp, vp, vp, vp, sz, dp, vp, i64p],
        "ndt_map_remove_components": [vp, pp, fp_, C.POINTER(pkg.MapRemoveComponentsResult)],
    }
    for name in NEW:
        assert re.search(r"\b(int|void) %s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    assert L.ndt_map_components_default_params.restype is None and L.ndt_map_component_filter_default_params.restype is None
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))

    def types_of(name):
        args = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, flat).group(1).split(",")
        out = []
        for a in args:
            a = a.strip()
            a = re.sub(r"\s*\b[a-z_0-9]+$", "", a) if not a.endswith("*") else a        # drop the parameter's name
            out.append(a.replace(" *", "*"))
        return out

    P = "const ndt_map_components_params*"
    assert types_of("ndt_map_components_default_params") == ["ndt_map_components_params*"]
    assert types_of("ndt_map_component_filter_default_params") == ["ndt_map_component_filter*"]
    assert types_of("ndt_map_components") == ["ndt_handle*", P, "ndt_map_components_info*"]
    assert types_of("ndt_map_export_components") == ["ndt_handle*", P, "ndt_map_component*", "size_t", "size_t*"]
    for name in ("ndt_map_export_labels", "ndt_map_export_labels_device"):
        assert types_of(name) == ["ndt_handle*", P, "int32_t*", "int32_t*", "size_t", "size_t*"], name
    assert types_of("ndt_map_label_points") == ["ndt_handle*", P, "const float*", "size_t", "size_t", "const double*", "int32_t*",
                                                "int64_t*"]
    assert types_of("ndt_map_label_points_device") == ["ndt_handle*", P, "const float*", "const float*", "const float*", "size_t",
                                                       "const double*", "int32_t*", "int64_t*"]
    assert types_of("ndt_map_remove_components") == ["ndt_handle*", P, "const ndt_map_component_filter*",
                                                     "ndt_map_remove_components_result*"]
    assert "typedef struct ndt_map_components_params { int connectivity; int min_count; int reserved[2]; } ndt_map_components_params;" in flat
    assert ("typedef struct ndt_map_component { int32_t root_ijk[3]; int32_t n_voxels; int64_t n_points; int32_t min_ijk[3], "
            "max_ijk[3]; } ndt_map_component;") in flat
    assert ("typedef struct ndt_map_components_info { int64_t n_components, n_voxels_labelled, n_voxels_unlabelled; int64_t largest; "
            "int64_t largest_n_voxels, largest_n_points; } ndt_map_components_info;") in flat
    assert ("typedef struct ndt_map_component_filter { int32_t min_voxels; int64_t min_points; int32_t keep_largest; "
            "int32_t remove_unlabelled; int32_t dry_run; int32_t reserved[3]; } ndt_map_component_filter;") in flat
    assert ("typedef struct ndt_map_remove_components_result { int64_t n_components, n_components_removed, n_removed, "
            "n_points_removed; } ndt_map_remove_components_result;") in flat
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    assert re.search(r"NDT_ERR_INTERNAL = -10\b", hdr)
    assert (C.sizeof(pkg.MapComponentsParams), C.sizeof(pkg.MapComponent), C.sizeof(pkg.MapComponentsInfo),
            C.sizeof(pkg.MapComponentFilter), C.sizeof(pkg.MapRemoveComponentsResult)) == (16, 48, 48, 40, 32)
    assert pkg.MapComponent.n_points.offset == 16 and pkg.MapComponent.min_ijk.offset == 24
    assert pkg.MapComponentFilter.min_points.offset == 8 and pkg.MapComponentFilter.keep_largest.offset == 16
    assert [f for f, _ in pkg.MapComponentsInfo._fields_] == list(INFO_FIELDS)
    assert [f for f, _ in pkg.MapRemoveComponentsResult._fields_] == list(REMOVE_FIELDS)
    assert [f for f, _ in pkg.MapComponent._fields_] == list(COMP_FIELDS)
    # the declarations stand beside the carve block
    assert hdr.index("int ndt_map_carve_keyframe(") < hdr.index("typedef struct ndt_map_components_params") < hdr.index("int ndt_map_transform(")
    hpp = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    for m in ("mapComponents", "mapExportComponents", "mapExportLabels", "mapExportLabelsDevice", "mapLabelPoints",
              "mapLabelPointsDevice", "mapRemoveComponents"):
        assert callable(getattr(pkg, m)), m
        assert re.search(r"\b%s\s*\(" % m, hpp), m
    assert hpp.index("mapCarveKeyframe(") < hpp.index("mapComponents(")


def test_defaults(pkg):
    L = pkg.lib()
    p = pkg.MapComponentsParams(9, 9, (9, 9))
    L.ndt_map_components_default_params(C.byref(p))
    assert (p.connectivity, p.min_count, list(p.reserved)) == (26, 1, [0, 0])
    f = pkg.MapComponentFilter(9, 9, 9, 9, 9, (9, 9, 9))
    L.ndt_map_component_filter_default_params(C.byref(f))
    assert (f.min_voxels, f.min_points, f.keep_largest, f.remove_unlabelled, f.dry_run, list(f.reserved)) == (1, 0, 0, 0, 0, [0, 0, 0])
    L.ndt_map_components_default_params(None)                                                  # (nothing to write: no crash)
    L.ndt_map_component_filter_default_params(None)


def test_argument_errors_come_before_the_handle(pkg):
    L = pkg.lib()
    n_dev, _ = pkg.backend_info()
    if n_dev <= 0:
        with pytest.raises(pkg.NdtError) as ei:
            pkg.mapComponents(pkg.NormalDistributionsTransform())
        assert ei.value.code == -2                           # NDT_ERR_NO_DEVICE: no CPU fallback
    f32 = (C.c_float * 64)()
    lab = (C.c_int32 * 64)(*([7] * 64))
    comps = (pkg.MapComponent * 4)()
    pose = (C.c_double * 16)(*np.eye(4).ravel())
    n_out, n_lab = C.c_size_t(7), C.c_int64(7)
    info = pkg.MapComponentsInfo(7, 7, 7, 7, 7, 7)
    res = pkg.MapRemoveComponentsResult(7, 7, 7, 7)
    good, flt = pkg.MapComponentsParams(), pkg.MapComponentFilter()
    L.ndt_map_components_default_params(C.byref(good))
    L.ndt_map_component_filter_default_params(C.byref(flt))
    A = lambda a: C.cast(a, C.c_void_p)

    def forms(h, prm, filt=C.byref(flt), pose_=pose):
        return (L.ndt_map_components(h, prm, C.byref(info)),
                L.ndt_map_export_components(h, prm, comps, 4, C.byref(n_out)),
                L.ndt_map_export_labels(h, prm, A(lab), A(lab), 4, C.byref(n_out)),
                L.ndt_map_export_labels_device(h, prm, A(lab), A(lab), 4, C.byref(n_out)),
                L.ndt_map_label_points(h, prm, A(f32), 4, 12, pose_, A(lab), C.byref(n_lab)),
                L.ndt_map_label_points_device(h, prm, A(f32), A(f32), A(f32), 4, pose_, A(lab), C.byref(n_lab)),
                L.ndt_map_remove_components(h, prm, filt, C.byref(res)))

    bad7 = (-1,) * 7
    assert forms(None, C.byref(good)) == bad7                                                  # NULL handle
    # the argument checks come before the handle is looked at: a stand-in block of zero bytes is never read
    h = C.create_string_buffer(1 << 16)
    assert forms(h, None) == bad7                                                              # NULL params
    for field, value in (("connectivity", 0), ("connectivity", 7), ("connectivity", 27), ("connectivity", -6), ("min_count", 0),
                         ("min_count", -1)):
        p = pkg.MapComponentsParams()
        L.ndt_map_components_default_params(C.byref(p))
        setattr(p, field, value)
        assert forms(h, C.byref(p)) == bad7, (field, value)
    for k in range(2):
        p = pkg.MapComponentsParams()
        L.ndt_map_components_default_params(C.byref(p))
        p.reserved[k] = 1
        assert forms(h, C.byref(p)) == bad7, k
    g = C.byref(good)
    assert L.ndt_map_remove_components(h, g, None, C.byref(res)) == -1                          # NULL filter
    for field, value in (("min_voxels", 0), ("min_voxels", -2), ("min_points", -1), ("keep_largest", -1)):
        f = pkg.MapComponentFilter()
        L.ndt_map_component_filter_default_params(C.byref(f))
        setattr(f, field, value)
        assert L.ndt_map_remove_components(h, g, C.byref(f), C.byref(res)) == -1, (field, value)
    for k in range(3):
        f = pkg.MapComponentFilter()
        L.ndt_map_component_filter_default_params(C.byref(f))
        f.reserved[k] = 1
        assert L.ndt_map_remove_components(h, g, C.byref(f), C.byref(res)) == -1, k
    for k in (0, 5, 15):                                                                       # a pose that is not finite
        for v in (float("nan"), float("inf")):
            bad = (C.c_double * 16)(*np.eye(4).ravel())
            bad[k] = v
            assert L.ndt_map_label_points(h, g, A(f32), 4, 12, bad, A(lab), C.byref(n_lab)) == -1, (k, v)
            assert L.ndt_map_label_points_device(h, g, A(f32), A(f32), A(f32), 4, bad, A(lab), C.byref(n_lab)) == -1, (k, v)
    assert L.ndt_map_label_points(h, g, None, 4, 12, None, A(lab), C.byref(n_lab)) == -1         # no cloud
    assert L.ndt_map_label_points(h, g, A(f32), 4, 12, None, None, C.byref(n_lab)) == -1         # no label output
    for stride in (8, 14):
        assert L.ndt_map_label_points(h, g, A(f32), 4, stride, None, A(lab), C.byref(n_lab)) == -1
    for hole in range(3):
        ptrs = [A(f32)] * 3
        ptrs[hole] = None
        assert L.ndt_map_label_points_device(h, g, *ptrs, 4, None, A(lab), C.byref(n_lab)) == -1
    assert L.ndt_map_label_points_device(h, g, A(f32), A(f32), A(f32), 4, None, None, C.byref(n_lab)) == -1
    assert L.ndt_map_export_components(h, g, comps, 4, None) == -1                              # nowhere to report the size
    assert L.ndt_map_export_components(h, g, None, 4, C.byref(n_out)) == -1
    assert L.ndt_map_export_labels(h, g, A(lab), A(lab), 4, None) == -1
    assert L.ndt_map_export_labels_device(h, g, A(lab), A(lab), 4, None) == -1
    # nothing was written
    assert [getattr(info, k) for k in INFO_FIELDS] == [7] * 6 and [getattr(res, k) for k in REMOVE_FIELDS] == [7] * 4
    assert n_out.value == 7 and n_lab.value == 7 and list(lab) == [7] * 64 and bytes(h.raw) == bytes(1 << 16)


def test_python_mirror_validates_before_the_library(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)   # no handle: nothing may reach the library
    ndt._h = None
    cloud = np.zeros((4, 3), np.float32)
    nan_pose = np.eye(4)
    nan_pose[1, 3] = np.nan
    bad = [
        lambda: pkg.mapComponents(ndt, connectivity=8), lambda: pkg.mapComponents(ndt, min_count=0),
        lambda: pkg.mapExportComponents(ndt, connectivity=0), lambda: pkg.mapExportLabels(ndt, connectivity=27),
        lambda: pkg.mapExportLabelsDevice(ndt, 0, 0, 4, min_count=-1),
        lambda: pkg.mapLabelPoints(ndt, cloud, connectivity=4), lambda: pkg.mapLabelPoints(ndt, np.zeros((4, 2), np.float32)),
        lambda: pkg.mapLabelPoints(ndt, cloud, pose=np.eye(3)), lambda: pkg.mapLabelPoints(ndt, cloud, pose=nan_pose),
        lambda: pkg.mapLabelPointsDevice(ndt, 1, 1, 1, 4, 1, pose=nan_pose), lambda: pkg.mapLabelPointsDevice(ndt, 1, 1, 1, 4, None),
        lambda: pkg.mapLabelPointsDevice(ndt, 1, None, 1, 4, 1),
        lambda: pkg.mapRemoveComponents(ndt, min_voxels=0), lambda: pkg.mapRemoveComponents(ndt, min_points=-1),
        lambda: pkg.mapRemoveComponents(ndt, keep_largest=-1), lambda: pkg.mapRemoveComponents(ndt, connectivity=5),
        lambda: pkg.mapRemoveComponents(ndt, min_voxels=2 ** 31), lambda: pkg.mapRemoveComponents(ndt, min_points=2 ** 63),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d reached the library" % k)


# ---- the restatement against hand-worked cases --------------------------------------------------------------------------
def labels_of(vox, counts=None, connectivity=26, min_count=1):
    """{voxel: label} of the restatement"""
    vox = np.asarray(vox, np.int64).reshape(-1, 3)
    cc = components_numpy(vox, np.ones(len(vox), np.int64) if counts is None else counts, connectivity, min_count)
    return {tuple(v): int(l) for v, l in zip(cc["ijk"].tolist(), cc["label"])}, cc


def test_offsets_are_the_three_neighbourhoods():
    assert [len(offsets_of(c)) for c in CONNECTIVITIES] == [6, 18, 26]
    assert set(offsets_of(6)) < set(offsets_of(18)) < set(offsets_of(26))
    for c in CONNECTIVITIES:
        assert all((-a, -b, -d) in offsets_of(c) for a, b, d in offsets_of(c))       # symmetric: adjacency is mutual
        # the forward half, the offsets with the larger key: 3, 9, 13
        assert sum(1 for o in offsets_of(c) if (o[2], o[1], o[0]) > (0, 0, 0)) == c // 2


def test_hand_worked_cases():
    # nothing and one voxel
    cc = components_numpy(np.zeros((0, 3)), np.zeros(0))
    assert cc["info"] == dict(n_components=0, n_voxels_labelled=0, n_voxels_unlabelled=0, largest=-1, largest_n_voxels=0,
                              largest_n_points=0) and len(cc["label"]) == 0
    lab, cc = labels_of([(3, -4, 5)], counts=[7])
    assert lab == {(3, -4, 5): 0} and cc["info"]["largest_n_points"] == 7
    assert cc["comps"]["root_ijk"].tolist() == [[3, -4, 5]] and cc["comps"]["min_ijk"].tolist() == cc["comps"]["max_ijk"].tolist() == [[3, -4, 5]]
    # two voxels: by a face, an edge, a corner, apart -- components under 6, 18, 26
    for other, want in (((1, 0, 0), (1, 1, 1)), ((0, 0, -1), (1, 1, 1)), ((1, 1, 0), (2, 1, 1)), ((0, -1, 1), (2, 1, 1)),
                        ((1, 1, 1), (2, 2, 1)), ((-1, 1, -1), (2, 2, 1)), ((2, 0, 0), (2, 2, 2)), ((1, 1, 2), (2, 2, 2))):
        for c, n in zip(CONNECTIVITIES, want):
            assert labels_of([(0, 0, 0), other], connectivity=c)[1]["info"]["n_components"] == n, (other, c)
    # numbering follows the roots in (k, j, i) order, whatever the input order: k first, then j, then i
    vox = [(5, 5, 1), (0, 0, 2), (9, 0, 0), (0, 1, 0), (1, 1, 0)]
    lab, cc = labels_of(vox, connectivity=6)
    assert lab == {(9, 0, 0): 0, (0, 1, 0): 1, (1, 1, 0): 1, (5, 5, 1): 2, (0, 0, 2): 3}
    assert cc["ijk"].tolist() == [[9, 0, 0], [0, 1, 0], [1, 1, 0], [5, 5, 1], [0, 0, 2]]
    assert cc["comps"]["root_ijk"].tolist() == [[9, 0, 0], [0, 1, 0], [5, 5, 1], [0, 0, 2]]
    assert labels_of(vox[::-1], connectivity=6)[0] == lab
    # an L of four voxels and a far one: record fields, and the largest is the FIRST of the largest
    vox = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (7, 7, 7), (8, 7, 7), (8, 8, 7), (8, 8, 8)]
    counts = [1, 2, 3, 4, 5, 5, 5, 5]
    lab, cc = labels_of(vox, counts, connectivity=6)
    assert cc["comps"]["n_voxels"].tolist() == [4, 4] and cc["comps"]["n_points"].tolist() == [10, 20]
    assert cc["comps"]["min_ijk"].tolist() == [[0, 0, 0], [7, 7, 7]] and cc["comps"]["max_ijk"].tolist() == [[1, 1, 1], [8, 8, 8]]
    assert cc["info"] == dict(n_components=2, n_voxels_labelled=8, n_voxels_unlabelled=0, largest=0, largest_n_voxels=4, largest_n_points=10)
    # min_count: a bridge with too few points joins nothing and has label -1
    vox = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0)]
    counts = [3, 3, 1, 3, 3]
    assert set(labels_of(vox, counts, 6, 1)[0].values()) == {0}
    lab, cc = labels_of(vox, counts, 6, 2)
    assert lab == {(0, 0, 0): 0, (1, 0, 0): 0, (2, 0, 0): -1, (3, 0, 0): 1, (4, 0, 0): 1}
    assert cc["info"]["n_voxels_unlabelled"] == 1 and cc["comps"]["n_points"].tolist() == [6, 6]
    # the edge of the coordinate range: no wrap from one end of an axis to the other
    e = LIMIT - 1
    lab, _ = labels_of([(e, 0, 0), (-e, 1, 0), (e - 1, 0, 0), (-e, -e, -e), (-e + 1, -e, -e)], connectivity=26)
    assert lab[(e, 0, 0)] == lab[(e - 1, 0, 0)] != lab[(-e, 1, 0)] and lab[(-e, -e, -e)] == lab[(-e + 1, -e, -e)] == 0
    # the checkerboard: faces never touch, edges always do
    g = np.array([(i, j, k) for k in range(8) for j in range(8) for i in range(8) if (i + j + k) % 2 == 0])
    assert [labels_of(g, connectivity=c)[1]["info"]["n_components"] for c in CONNECTIVITIES] == [256, 1, 1]


def test_the_snake_is_one_component_as_long_as_itself():
    path = snake_path(4096)
    assert len(path) == 4096 and len(np.unique(state_key(path))) == 4096
    at = {tuple(v): r for r, v in enumerate(path.tolist())}                # the only face adjacencies: consecutive voxels
    pairs = 0
    for r, (i, j, k) in enumerate(path.tolist()):
        for n in ((i + 1, j, k), (i - 1, j, k), (i, j + 1, k), (i, j - 1, k), (i, j, k + 1), (i, j, k - 1)):
            if n in at:
                assert abs(at[n] - r) == 1, (r, at[n])
                pairs += 1
    assert pairs == 2 * 4095
    cc = components_numpy(path, np.ones(4096), 6)
    assert cc["info"]["n_components"] == 1 and cc["info"]["largest_n_voxels"] == 4096
    cut = np.delete(path, 2048, axis=0)
    cc = components_numpy(cut, np.ones(4095), 6)
    assert cc["info"]["n_components"] == 2 and sorted(cc["comps"]["n_voxels"].tolist()) == [2047, 2048]


def test_restatement_against_scipy_on_a_dense_box():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    for fill in (0.15, 0.3, 0.6):
        vol = rng.random((14, 13, 12)) < fill                                # indexed [k, j, i]
        k, j, i = np.nonzero(vol)
        ijk = np.stack([i, j, k], 1) - 5                                     # (negative coordinates as well)
        for c, rank in zip(CONNECTIVITIES, (1, 2, 3)):
            lab, n = ndimage.label(vol, structure=ndimage.generate_binary_structure(3, rank))
            cc = components_numpy(ijk, np.ones(len(ijk)), c)
            assert cc["info"]["n_components"] == n
            # the same partition (scipy numbers in scan order of [k, j, i], which is the rule's order as well)
            mine = cc["label"]
            theirs = lab[cc["ijk"][:, 2] + 5, cc["ijk"][:, 1] + 5, cc["ijk"][:, 0] + 5] - 1
            assert np.array_equal(mine, theirs)


def test_remove_numpy_on_hand_worked_components():
    # sizes 3, 1, 3, 2 in index order, points 3, 9, 6, 2; one ineligible voxel
    vox = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (5, 0, 0), (0, 5, 0), (1, 5, 0), (2, 5, 0), (0, 0, 5), (1, 0, 5), (9, 9, 9)]
    counts = np.array([2, 2, 2, 9, 2, 2, 2, 2, 2, 1])
    cc = components_numpy(vox, counts, 6, 2)
    assert cc["comps"]["n_voxels"].tolist() == [3, 1, 3, 2] and cc["label"][-1] == -1
    info0 = dict(n_voxels=10, n_points=int(counts.sum()), capacity=64, min_ijk=(0, 0, 0), max_ijk=(9, 9, 9), reset_capacity=64)
    assert survivors_numpy(cc["comps"]).all()
    r = remove_numpy(cc, info0)                                              # the default filter removes nothing
    assert r["result"] == dict(n_components=4, n_components_removed=0, n_removed=0, n_points_removed=0) and r["keep"].all() and r["info"] == info0
    assert survivors_numpy(cc["comps"], min_voxels=2).tolist() == [True, False, True, True]
    assert survivors_numpy(cc["comps"], min_points=6).tolist() == [True, True, True, False]
    assert survivors_numpy(cc["comps"], keep_largest=1).tolist() == [True, False, False, False]    # the lower index of the equal two
    assert survivors_numpy(cc["comps"], keep_largest=2).tolist() == [True, False, True, False]
    assert survivors_numpy(cc["comps"], keep_largest=3).tolist() == [True, False, True, True]
    assert survivors_numpy(cc["comps"], keep_largest=9).all()
    # the position counts ALL components: the second largest does not move up when min_points rejects the first
    assert survivors_numpy(cc["comps"], min_points=7, keep_largest=1).tolist() == [False, False, False, False]
    r = remove_numpy(cc, info0, min_voxels=2, remove_unlabelled=True)
    assert r["result"] == dict(n_components=4, n_components_removed=1, n_removed=2, n_points_removed=10)
    assert r["info"]["n_voxels"] == 8 and r["info"]["n_points"] == 16 and r["info"]["max_ijk"] == (2, 5, 5) and r["info"]["capacity"] == 64
    r = remove_numpy(cc, info0, remove_unlabelled=True)
    assert r["result"]["n_removed"] == 1 and r["result"]["n_components_removed"] == 0 and not r["keep"][-1] and r["keep"][:-1].all()
    d = remove_numpy(cc, info0, min_voxels=2, dry_run=True)
    assert d["result"]["n_removed"] == 1 and d["keep"].all() and d["info"] == info0
    r = remove_numpy(cc, info0, min_voxels=4, remove_unlabelled=True)        # everything goes: the box is left as it was
    assert r["info"]["n_voxels"] == 0 and r["info"]["n_points"] == 0 and r["info"]["min_ijk"] == (0, 0, 0)


def test_map_hash_numpy_is_splitmix64s_finaliser():
    # the finaliser's published test values: mix(0) = 0, and the first outputs of splitmix64 seeded with 0 are the
    # finaliser of 0x9e3779b97f4a7c15 and of twice that
    got = map_hash_numpy(np.array([0, 0x9e3779b97f4a7c15, (2 * 0x9e3779b97f4a7c15) % 2 ** 64], np.uint64))
    assert [int(v) for v in got] == [0, 0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4]


# ---- the kernels --------------------------------------------------------------------------------------------------------
KERNELS = {"k_mapcc_init", "k_mapcc_link", "k_mapcc_flatten", "k_mapcc_rootcount", "k_mapcc_number", "k_mapcc_reduce",
           "k_mapcc_gather", "k_mapcc_points", "k_mapcc_move"}


def test_map_components_kernels_do_not_spill(tmp_path):
    path = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_map_components.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    assert usage and all("k_mapcc_" in k for k in usage), sorted(usage)
    table = {re.search(r"k_mapcc_[a-z]+", k).group(0): u for k, u in usage.items()}
    assert set(table) == KERNELS, sorted(table)
    for k, u in table.items():
        assert u["ScratchSize"] == 0, (k, u)
    lines = ["kernel resources of slam-sam_amd/csrc/ndt_map_components.hip (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off,",
             "-Rpass-analysis=kernel-resource-usage; written by tests/test_map_components_cpu.py)", "",
             "%-20s %6s %6s %8s %6s" % ("kernel", "VGPRs", "SGPRs", "scratch", "LDS")]
    for k in sorted(table):
        u = table[k]
        lines.append("%-20s %6d %6d %8d %6d" % (k, u["VGPRs"], u["TotalSGPRs"], u["ScratchSize"], u["LDS"]))
    try:
        with open(os.path.join(ROOT, "profiles", "map_components_resources.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                                                 # (a read-only checkout: the table is in git)
    src = open(path).read()
    assert len(re.findall(r"__global__ void __launch_bounds__\(MAP_THREADS\)", src)) == len(re.findall(r"__global__", src)) == len(KERNELS)
    # integer atomics only, no inline assembly; the shared compaction, probe and move, no copies of them
    assert not re.search(r"atomicAdd\([^;]*float|unsafeAtomicAdd|\basm\b|__asm", src)
    for shared in ('#include "ndt_compact_device.h"', '#include "ndt_map_device.h"', "map_find(", "compact_ballot(", "compact_position(",
                   "launch_filter_scan(", "map_export_order(", "map_move_slot(", "map_grow_table("):
        assert shared in src, shared
    # the hook is a CAS, and a failed one goes on from what it returned
    assert re.search(r"const uint32_t old = atomicCAS\(parent \+ rb, rb, ra\);", src) and "cc_find(parent, old, cap)" in src
    assert "$(B)/ndt_map_components.o" in open(os.path.join(ROOT, "slam-sam_amd", "csrc", "Makefile")).read()
