"""CPU checks of the voxel-map boundary (no GPU): the new C-ABI symbols are declared, exported and bound with their
signatures; bad arguments are refused before a device (or the handle) is touched; without a device nothing computes
(NDT_ERR_NO_DEVICE); the NumPy yardstick of tests/test_gpu_voxel_map.py agrees with PCL's dense-index restatement where
both apply; the map's kernels compile for gfx950 without scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_map_reset", "ndt_map_clear", "ndt_map_add", "ndt_map_add_device", "ndt_map_add_keyframe", "ndt_map_get_info",
       "ndt_map_export_device", "ndt_map_export", "ndt_set_target_from_map")


def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    want = {
        "ndt_map_reset": [vp, C.c_float, C.c_int, C.c_int64],
        "ndt_map_clear": [vp],
        "ndt_map_add": [vp, vp, C.c_size_t, C.c_size_t, C.c_long, dp],
        "ndt_map_add_device": [vp, vp, vp, vp, vp, C.c_size_t, dp],
        "ndt_map_add_keyframe": [vp, C.c_int64, dp],
        "ndt_map_get_info": [vp, C.POINTER(pkg.MapInfo)],
        "ndt_map_export_device": [vp, C.c_int, vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)],
        "ndt_map_export": [vp, C.c_int, vp, C.c_size_t, C.c_long, vp, C.c_size_t, C.POINTER(C.c_size_t)],
        "ndt_set_target_from_map": [vp, C.c_int],
    }
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    # the declared parameter lists, as the issue gives them
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int ndt_map_reset(ndt_handle* h, float leaf, int with_intensity, int64_t initial_capacity);" in flat
    assert ("int ndt_map_add(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, long intensity_offset_bytes, "
            "const double* pose16_colmajor_or_null);") in flat
    assert "int ndt_map_get_info(const ndt_handle* h, ndt_map_info* out);" in flat
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    # the struct mirror: two 4-byte fields, four int64, six ints, two int64
    assert C.sizeof(pkg.MapInfo) == 8 + 4 * 8 + 6 * 4 + 2 * 8
    for m in ("mapReset", "mapClear", "mapAdd", "mapAddDevice", "mapAddKeyframe", "mapInfo", "mapExport", "mapExportDevice",
              "setInputTargetFromMap"):
        assert callable(getattr(pkg.NormalDistributionsTransform, m)), m
        assert re.search(r"\b%s\s*\(" % m, open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()), m


def test_argument_errors_and_no_device(pkg):
    L = pkg.lib()
    n, info = pkg.backend_info()
    if n <= 0:
        with pytest.raises(pkg.NdtError) as ei:
            pkg.NormalDistributionsTransform().mapReset(0.5)
        assert ei.value.code == -2                           # NDT_ERR_NO_DEVICE: no CPU fallback
    f = (C.c_float * 64)()
    cnt = (C.c_int32 * 8)()
    m = C.c_size_t(7)
    mi = pkg.MapInfo()
    # NULL handle
    assert L.ndt_map_reset(None, 0.5, 0, 0) == -1
    assert L.ndt_map_clear(None) == -1
    assert L.ndt_map_add(None, f, 4, 16, -1, None) == -1
    assert L.ndt_map_add_device(None, None, None, None, None, 0, None) == -1
    assert L.ndt_map_add_keyframe(None, 1, None) == -1
    assert L.ndt_map_get_info(None, C.byref(mi)) == -1
    assert L.ndt_map_export_device(None, 1, None, None, None, None, None, 0, C.byref(m)) == -1
    assert L.ndt_map_export(None, 1, f, 16, -1, cnt, 4, C.byref(m)) == -1
    assert L.ndt_set_target_from_map(None, 1) == -1
    # the argument checks come before the handle is looked at: a stand-in block of zero bytes is never read
    h = C.create_string_buffer(1 << 16)
    for leaf in (0.0, 1e-6, -1.0, float("nan"), float("inf")):
        assert L.ndt_map_reset(h, leaf, 0, 0) == -1
    assert L.ndt_map_reset(h, 0.5, 0, -1) == -1
    for stride, off in ((8, -1), (14, -1), (16, 3), (16, 13), (16, 8), (16, 16), (20, 20)):
        assert L.ndt_map_add(h, f, 2, stride, off, None) == -1, (stride, off)
        assert L.ndt_map_export(h, 1, f, stride, off, cnt, 2, C.byref(m)) == -1, (stride, off)
    assert L.ndt_map_add(h, None, 2, 16, -1, None) == -1
    assert L.ndt_map_add_device(h, None, None, None, None, 2, None) == -1
    assert L.ndt_map_add_keyframe(h, 1, None) == -1
    assert L.ndt_map_export(h, 1, f, 16, -1, cnt, 2, None) == -1
    assert L.ndt_map_export_device(h, 1, None, None, None, None, None, 2, C.byref(m)) == -1
    assert L.ndt_map_get_info(h, None) == -1
    assert m.value == 7 and bytes(h.raw) == bytes(1 << 16)   # nothing was written


def test_python_mirror_validates_its_arguments(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)
    ndt._h = C.c_void_p()
    for call in (lambda: ndt.mapAdd(np.zeros((4, 2), np.float32)), lambda: ndt.mapAdd(np.zeros((4, 3), np.float32), pose=np.eye(3)),
                 lambda: ndt.mapAddKeyframe(1, None), lambda: ndt.mapExport(columns=2),
                 lambda: ndt.mapExport(columns=4, intensity_column=4)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(pkg.NdtError) as ei:                  # a NULL handle reaches the C call and is refused there
        ndt.mapInfo()
    assert ei.value.code == -1


def voxelgrid_dense_numpy(pts, leaf):
    """PCL VoxelGrid::applyFilter restated with its dense index (min_b of the bounding box, f32 subtraction)."""
    q = np.asarray(pts, np.float32)
    q = q[np.isfinite(q).all(axis=1)]
    inv = np.float32(1.0) / np.float32(leaf)
    min_b = np.floor(q.min(0) * inv).astype(np.int64)
    div_b = np.floor(q.max(0) * inv).astype(np.int64) - min_b + 1
    ijk = (np.floor(q * inv) - min_b.astype(np.float32)).astype(np.int64)
    flat = ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * div_b[0] * div_b[1]
    order = np.argsort(flat, kind="stable")
    fs = flat[order]
    heads = np.nonzero(np.r_[True, fs[1:] != fs[:-1]])[0]
    counts = np.diff(np.r_[heads, len(fs)])
    out = np.zeros((len(heads), 3), np.float32)
    for r, (h0, c) in enumerate(zip(heads, counts)):
        acc = np.zeros(3, np.float32)
        for j in range(c):
            acc = acc + q[order[h0 + j]]
        out[r] = acc / np.float32(c)
    return out, counts


def test_the_sparse_yardstick_agrees_with_the_dense_index():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gpu_voxel_map_yardstick", os.path.join(ROOT, "tests", "test_gpu_voxel_map.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(1)
    cloud = rng.uniform([-3, -2, -1], [3, 2, 1], (3000, 3)).astype(np.float32)
    cloud[::97] = np.nan
    cloud[5] = [-0.0, 0.5, -0.5]
    for leaf in (0.5, 0.3):
        xyz, _, counts, ijk = mod.voxelmap_numpy(cloud, leaf)
        dense, dcounts = voxelgrid_dense_numpy(cloud, leaf)
        assert np.array_equal(xyz.view(np.uint32), dense.view(np.uint32)) and np.array_equal(counts, dcounts)
        assert np.array_equal(ijk, ijk[np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))]) and len(np.unique(ijk, axis=0)) == len(ijk)
    # a pose is applied in f64 and rounded once
    T = np.eye(4)
    T[:3, 3] = [1e-9, 0.25, -3.0]
    some = cloud[1:11]                                       # (finite rows)
    moved = mod.host_transform_f64(T, some)
    assert moved.dtype == np.float32 and np.array_equal(moved[:, 1], (some[:, 1].astype(np.float64) + 0.25).astype(np.float32))


def test_map_kernels_do_not_spill(tmp_path):
    """The figures tools/kernel_resources.py prints for `ndt_map.hip k_map_`: every kernel of the map without scratch."""
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_map.hip"),
                        "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", ln)
        if m and name and "k_map_" in name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    kernels = {re.search(r"k_map_[a-z]+", k).group(0) for k in usage}
    assert kernels == {"k_map_keys", "k_map_insert", "k_map_accumulate", "k_map_rehash", "k_map_xcount", "k_map_xemit",
                       "k_map_xgather", "k_map_xcentroids"}, kernels
    for k, u in usage.items():
        assert u["ScratchSize"] == 0, (k, u)
    src = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_map.hip")).read()
    assert len(re.findall(r"__global__ void __launch_bounds__\(", src)) == len(re.findall(r"__global__", src)) == len(kernels)
    # no floating-point atomics, no inline assembly
    assert not re.search(r"atomicAdd\([^;]*float|unsafeAtomicAdd|\basm\b", src)


def test_the_table_move_has_one_definition():
    """The key's layout, a slot's move into a fresh table, the block's reduction of an ijk box and the 64-bit wave sum are
    defined in ndt_map_device.h and nowhere else; growth, crop and carve call the move and replace the table through ONE
    host function."""
    csrc = os.path.join(ROOT, "slam-sam_amd", "csrc")
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip", ".cpp"))}
    maps = ("ndt_map.hip", "ndt_map_state.hip", "ndt_map_carve.hip")
    for fn in ("map_key", "map_ijk", "map_move_slot", "map_box_waves", "map_box_commit", "wave_sum_u64"):
        defs = [f for f, text in sources.items() if re.search(r"\b(unsigned long long|void|bool) %s\(" % fn, text)]
        assert defs == ["ndt_map_device.h"], (fn, defs)
    for f in maps:
        assert re.search(r"\bmap_move_slot\(", sources[f]), f
    # nobody else writes the key's arithmetic or the box's atomics out
    for f, text in sources.items():
        if f != "ndt_map_device.h":
            assert "0x1fffff" not in text.lower() and "<< 42" not in text, f
    for f in maps:
        assert "atomicMin(" not in sources[f] and "atomicMax(" not in sources[f], f
    assert "atomicMin(" in sources["ndt_map_device.h"] and "atomicMax(" in sources["ndt_map_device.h"]

    def callers(fn):
        """(file, enclosing function) of every call of fn: the nearest definition line above it that starts in column 0"""
        out = []
        for f, text in sources.items():
            for m in re.finditer(r"\b%s\(" % fn, text):
                line_start = text.rfind("\n", 0, m.start()) + 1
                if re.match(r"(int|void) %s\(" % fn, text[line_start:]):        # its own definition / declaration
                    continue
                heads = re.findall(r"^(?:int|void|bool) (\w+)\([^;]*?\) \{$", text[:m.start()], flags=re.M | re.S)
                out.append((f, heads[-1]))
        return sorted(out)

    assert callers("map_alloc_table") == [("ndt_map.hip", "map_replace_table"), ("ndt_map.hip", "ndt_map_reset")]
    assert callers("map_replace_table") == [("ndt_map.hip", "map_grow_table"), ("ndt_map_carve.hip", "map_carve_device"),
                                            ("ndt_map_state.hip", "map_crop")]
    everything = "\n".join(sources.values())
    for gone in ("carve_pose_finite", "carve_finite3", "carve_key", "box_finite"):
        assert not re.search(r"\b%s\b" % gone, everything), gone
    for fn in ("pose_finite", "finite3"):
        assert len(re.findall(r"^bool %s\(const" % fn, everything, flags=re.M)) == 2, fn      # declared once, defined once
