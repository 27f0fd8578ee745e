"""CPU checks of the voxel map's levels (ndt_map_level_info, ndt_map_export_state_level / _device,
ndt_set_target_from_map_level, ndt_map_coarsen, ndt_map_levels_drop, ndt_align_map_levels; no GPU).
The NumPy yardstick of the GPU tests lives here: `level_numpy(state, L)`, the rule of include/ndt_hip.h restated -- every
voxel goes to ijk >> L, a level voxel's fields start from +0 and add its children one at a time in ascending child
(k, j, i) order.  It is checked against the yardsticks the project already trusts (tests/test_map_state_cpu.py):
`merge_numpy`, of which it is the repeated application, and `mapstate_numpy` at the coarse leaf, which it must equal in
membership and counts on any cloud and in every bit on a cloud whose sums are exact.
Also here: the f32 identity the rule rests on, floor(p * inv_leaf_L) == floor(p * inv_leaf) >> L; the boundary (symbols,
struct sizes, argument checks before the handle); the kernels of ndt_map_levels.hip compile for gfx950 without scratch
and within 64 VGPRs (eight waves per SIMD)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_map_state_cpu import mapstate_numpy, merge_numpy, state_key, states_equal
from test_map_target_cpu import voxel_ijk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_map_level_info", "ndt_map_export_state_level", "ndt_map_export_state_level_device",
       "ndt_set_target_from_map_level", "ndt_map_coarsen", "ndt_map_levels_drop", "ndt_align_map_levels")
MAX_LEVEL = 6


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def level_leaf(leaf, L):
    """(float)(leaf * 2^L)"""
    return np.float32(np.float32(leaf) * np.float32(2 ** L))


def level_numpy(st, L):
    """Level L of the state `st` (a mapExportState dict: ascending (k, j, i)): ijk >> L, count summed, every f32 sum and
    f64 moment from +0 adding the children in ascending child (k, j, i) order, one rounding per add (vectorised over the
    level voxels, one child of every voxel per step).  Without intensity the intensity sum stays 0; without moments
    `moments` is None.  Ascending (k, j, i)."""
    ijk = np.asarray(st["ijk"], np.int32).reshape(-1, 3)
    assert np.all(np.diff(state_key(ijk)) > 0)                         # the children come in ascending order
    parent = ijk >> L                                                  # arithmetic: floor_div
    key = state_key(parent)
    order = np.argsort(key, kind="stable")                             # children of one parent stay in ascending order
    ks = key[order]
    heads = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0] if len(ks) else np.zeros(0, np.int64)
    n_child = np.diff(np.r_[heads, len(ks)])
    m = len(heads)
    count = np.zeros(m, np.int64)
    sums = np.zeros((m, 4), np.float32)
    with_mom = st.get("moments") is not None
    mom = np.zeros((m, 9), np.float64) if with_mom else None
    src_sums = np.asarray(st["sums"], np.float32).copy()
    if not st.get("with_intensity", True):
        src_sums[:, 3] = 0.0
    dst = np.arange(m)
    for j in range(int(n_child.max()) if m else 0):
        live = n_child > j
        src = order[heads[live] + j]
        sums[dst[live]] = sums[dst[live]] + src_sums[src]
        count[dst[live]] += np.asarray(st["count"], np.int64)[src]
        if with_mom:
            mom[dst[live]] = mom[dst[live]] + np.asarray(st["moments"], np.float64)[src]
    assert (count <= np.iinfo(np.int32).max).all(), "the level is refused: a count beyond INT32_MAX"
    return dict(leaf=float(level_leaf(st["leaf"], L)) if "leaf" in st else None,
                with_intensity=st.get("with_intensity", True), ijk=parent[order[heads]].astype(np.int32),
                count=count.astype(np.int32), sums=sums, moments=mom)


def level_by_merges(st, L):
    """the same through merge_numpy: an empty state that receives, round by round, the j-th child of every level voxel
    with its ijk shifted -- ndt_map_import_state's rule applied to the records in order"""
    ijk = np.asarray(st["ijk"], np.int32)
    parent = ijk >> L
    key = state_key(parent)
    rank = np.zeros(len(key), np.int64)                                # position of a child among its parent's children
    seen = {}
    for r, k in enumerate(key.tolist()):
        rank[r] = seen.get(k, 0)
        seen[k] = rank[r] + 1
    acc = dict(ijk=np.zeros((0, 3), np.int32), count=np.zeros(0, np.int32), sums=np.zeros((0, 4), np.float32),
               moments=np.zeros((0, 9), np.float64))
    for j in range(int(rank.max()) + 1 if len(rank) else 0):
        at = np.nonzero(rank == j)[0]
        at = at[np.argsort(key[at], kind="stable")]
        acc = merge_numpy(acc, dict(ijk=parent[at], count=st["count"][at], sums=st["sums"][at], moments=st["moments"][at]))
    return acc


def scene(n=6000, seed=3, quantum=None):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(-9.0, 9.0, (n, 3)), rng.normal(0.0, 0.4, (n // 4, 3)) + [2.2, -3.1, 0.4]])
    if quantum:
        pts = np.round(pts / quantum) * quantum
    return pts.astype(np.float32)


@pytest.mark.parametrize("leaf", [0.5, 0.3])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_level_numpy_is_the_repeated_merge(leaf, L):
    st = mapstate_numpy(scene(), leaf)
    st["leaf"] = leaf
    got, want = level_numpy(st, L), level_by_merges(st, L)
    assert len(got["count"]) < len(st["count"]) and int(got["count"].sum()) == int(st["count"].sum())
    assert states_equal(got, want)
    # ... and level 0 of the rule is the state itself
    assert states_equal(level_numpy(st, 0), st)


@pytest.mark.parametrize("leaf", [0.5, 0.3, 0.7])
@pytest.mark.parametrize("L", [1, 2, 4])
def test_level_numpy_holds_the_voxels_of_the_coarse_leaf(leaf, L):
    """membership and counts equal the map built from the points at leaf * 2^L, on any cloud"""
    pts = scene()
    st = mapstate_numpy(pts, leaf)
    st["leaf"] = leaf
    got = level_numpy(st, L)
    want = mapstate_numpy(pts, float(level_leaf(leaf, L)))
    assert np.array_equal(got["ijk"], want["ijk"]) and np.array_equal(got["count"], want["count"])
    # the sums differ by summation order only
    np.testing.assert_allclose(got["moments"], want["moments"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(got["sums"], want["sums"], rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("L", [1, 3])
def test_level_numpy_is_exact_on_a_quantised_cloud(L):
    """coordinates that are multiples of 2^-10 within +-10 m: every sum is exact in f64 (and in f32 here: below 2^14),
    whatever the order, so the level equals the map of the points at the coarse leaf in every bit"""
    leaf = 0.5
    pts = scene(quantum=2.0 ** -10)
    st = mapstate_numpy(pts, leaf)
    st["leaf"] = leaf
    got = level_numpy(st, L)
    want = mapstate_numpy(pts, float(level_leaf(leaf, L)))
    assert float(np.abs(want["sums"]).max()) < 2.0 ** 14
    assert states_equal(got, want)


def test_level_numpy_edge_cases():
    one = np.ones((3, 4), np.float32)
    st = dict(leaf=1.0, ijk=np.int32([[-1, 0, 0], [-2, 0, 0], [-3, 0, 0]])[::-1].copy(), count=np.int32([1, 2, 3]), sums=one,
              moments=np.ones((3, 9)))
    lv = level_numpy(st, 1)
    assert lv["ijk"].tolist() == [[-2, 0, 0], [-1, 0, 0]]            # -3 -> -2; -2, -1 -> -1
    assert lv["count"].tolist() == [1, 5] and lv["sums"][:, 0].tolist() == [1.0, 2.0]
    big = dict(leaf=1.0, ijk=np.int32([[0, 0, 0], [1, 0, 0]]), count=np.int32([2 ** 30, 2 ** 30]), sums=one[:2], moments=None)
    with pytest.raises(AssertionError):
        level_numpy(big, 1)
    plain = dict(leaf=1.0, with_intensity=False, ijk=np.int32([[0, 0, 0], [1, 1, 1]]), count=np.int32([1, 1]),
                 sums=np.float32([[1, 2, 3, 9], [1, 2, 3, 9]]), moments=None)
    lv = level_numpy(plain, 1)
    assert lv["moments"] is None and lv["sums"].tolist() == [[2.0, 4.0, 6.0, 0.0]]


# ---- the identity the rule rests on -------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [0.3, 0.7, 1.37])
def test_point_rule_identity_in_f32(leaf):
    """floor(p * inv_leaf_L) == floor(p * inv_leaf) >> L for L = 1 .. 4: random coordinates, the voxel faces k * leaf of
    both lattices and their f32 neighbours on either side"""
    rng = np.random.default_rng(11)
    lf = np.float32(leaf)
    inv = np.float32(1.0) / lf
    k = np.arange(-4096, 4097, dtype=np.float32)
    faces = [k * lf]
    for L in range(1, 5):
        faces.append(k * level_leaf(leaf, L))
    f = np.concatenate(faces)
    pts = np.concatenate([rng.uniform(-1200, 1200, 400000).astype(np.float32), f, np.nextafter(f, np.float32(np.inf)),
                          np.nextafter(f, np.float32(-np.inf)), np.float32([0.0, -0.0, 1e-30, -1e-30])])
    # the rule's own exception: a scaled coordinate that is subnormal (the neighbours of 0, |p| ~ 1e-45) may round to -0
    scaled = pts * inv
    normal = (scaled == 0) | (np.abs(scaled) >= np.finfo(np.float32).tiny)
    assert 0 < int((~normal).sum()) <= 32
    pts = pts[normal]
    fine = np.floor(pts * inv).astype(np.int64)
    for L in range(1, 5):
        ll = level_leaf(leaf, L)
        inv_l = np.float32(1.0) / ll
        assert inv_l == inv / np.float32(2 ** L)                       # 1.0f / (leaf * 2^L) is inv_leaf / 2^L exactly
        coarse = np.floor(pts * inv_l).astype(np.int64)
        assert np.array_equal(coarse, fine >> L), (leaf, L)
    # a factor that is no power of two has no such identity
    inv3 = np.float32(1.0) / (lf * np.float32(3.0))
    assert not np.array_equal(np.floor(pts * inv3).astype(np.int64), fine // 3)
    # voxel_ijk, the tests' own point rule, is the same arithmetic
    p3 = np.stack([pts[:1000]] * 3, axis=1)
    assert np.array_equal(voxel_ijk(p3, float(leaf))[:, 0], fine[:1000])


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, fp, sp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_size_t)
    want = {
        "ndt_map_level_info": [vp, C.c_int, C.POINTER(pkg.MapInfo)],
        "ndt_map_export_state_level": [vp, C.c_int, fp, fp, vp, vp, vp, vp, C.c_size_t, sp],
        "ndt_map_export_state_level_device": [vp, C.c_int, fp, fp, vp, vp, vp, vp, C.c_size_t, sp],
        "ndt_set_target_from_map_level": [vp, C.c_int, fp, fp],
        "ndt_map_coarsen": [vp, C.c_int],
        "ndt_map_levels_drop": [vp],
        "ndt_align_map_levels": [vp, C.POINTER(pkg.MapLevelStep), C.c_int, fp, fp, C.POINTER(pkg.Result)],
    }
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for decl in ("int ndt_map_level_info(ndt_handle* h, int level, ndt_map_info* out);",
                 "int ndt_set_target_from_map_level(ndt_handle* h, int level, const float box_min[3], const float box_max[3]);",
                 "int ndt_map_coarsen(ndt_handle* h, int level);", "int ndt_map_levels_drop(ndt_handle* h);",
                 "int ndt_align_map_levels(ndt_handle* h, const ndt_map_level_step* steps, int n_steps, "
                 "const float half_extent_or_null[3], const float guess_colmajor[16], ndt_result* results);",
                 "typedef struct ndt_map_level_step { int level; int max_iterations; double step_size; } ndt_map_level_step;"):
        assert decl in flat, decl
    assert re.search(r"#define NDT_MAP_MAX_LEVEL 6\b", hdr) and pkg.MAP_MAX_LEVEL == MAX_LEVEL
    assert re.search(r"#define NDT_MAP_LEVEL_STEPS_MAX 8\b", hdr) and pkg.MAP_LEVEL_STEPS_MAX == 8
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    assert C.sizeof(pkg.MapLevelStep) == 16 and pkg.MapLevelStep.step_size.offset == 8
    assert C.sizeof(pkg.MapInfo) == 80                                                # the level info is the map's struct
    hpp = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    for m in ("mapLevelInfo", "mapExportStateLevel", "mapExportStateLevelDevice", "setInputTargetFromMapLevel", "mapCoarsen",
              "mapLevelsDrop", "alignMapLevels"):
        assert re.search(r"\b%s\s*\(" % m, hpp), m
        assert callable(getattr(pkg, m)), m
    mk = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "Makefile")).read()
    assert "$(B)/ndt_map_levels.o" in mk


def test_argument_errors_come_before_the_handle(pkg):
    L = pkg.lib()
    info, n = pkg.MapInfo(), C.c_size_t(7)
    steps = (pkg.MapLevelStep * 2)()
    guess = (C.c_float * 16)()
    res = (pkg.Result * 2)()
    lo = (C.c_float * 3)()
    assert L.ndt_map_level_info(None, 1, C.byref(info)) == -1
    assert L.ndt_map_export_state_level(None, 1, None, None, None, None, None, None, 0, C.byref(n)) == -1
    assert L.ndt_map_export_state_level_device(None, 1, None, None, None, None, None, None, 0, C.byref(n)) == -1
    assert L.ndt_set_target_from_map_level(None, 1, None, None) == -1
    assert L.ndt_map_coarsen(None, 1) == -1 and L.ndt_map_levels_drop(None) == -1
    assert L.ndt_align_map_levels(None, steps, 2, None, guess, res) == -1
    # a stand-in block of zero bytes is never read
    h = C.create_string_buffer(1 << 16)
    assert L.ndt_map_level_info(h, 1, None) == -1
    for fn in (L.ndt_map_export_state_level, L.ndt_map_export_state_level_device):
        assert fn(h, 1, None, None, None, None, None, None, 0, None) == -1
        assert fn(h, 1, lo, None, None, None, None, None, 0, C.byref(n)) == -1       # half a box
    assert L.ndt_set_target_from_map_level(h, 1, None, lo) == -1
    assert L.ndt_align_map_levels(h, None, 2, None, guess, res) == -1
    assert L.ndt_align_map_levels(h, steps, 2, None, None, res) == -1
    assert L.ndt_align_map_levels(h, steps, 2, None, guess, None) == -1
    assert L.ndt_align_map_levels(h, steps, 0, None, guess, res) == -1
    assert L.ndt_align_map_levels(h, steps, 9, None, guess, res) == -1
    assert bytes(h.raw) == bytes(1 << 16) and n.value == 7


def test_python_mirror_validates_before_the_library(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)   # no handle: nothing may reach the library
    ndt._h = None
    bad = [
        lambda: pkg.mapExportStateLevel(ndt, 1, [0, 0, 0], None),
        lambda: pkg.mapExportStateLevelDevice(ndt, 1, 0, 0, 0, 0, 4, None, [0, 0, 0]),
        lambda: pkg.setInputTargetFromMapLevel(ndt, 1, [0, 0, np.nan], [1, 1, 1]),
        lambda: pkg.alignMapLevels(ndt, [2, 1, 0], half_extent=[1.0, 2.0]),
        lambda: pkg.alignMapLevels(ndt, [2, 1, 0], guess=np.eye(3)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d reached the library" % k)


# ---- the kernels --------------------------------------------------------------------------------------------------------
def test_maplevel_kernels_do_not_spill(tmp_path):
    """The figures tools/kernel_resources.py prints for `ndt_map_levels.hip k_maplevel_`: every kernel without scratch and
    within 64 VGPRs, the most a wave may hold at eight waves per SIMD (512 per lane and SIMD)."""
    path = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_map_levels.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", ln)
        if m and name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    assert usage and all("k_maplevel_" in k for k in usage), sorted(usage)            # the new kernels carry the prefix
    kernels = {re.search(r"k_maplevel_[a-z]+", k).group(0) for k in usage}
    assert kernels == {"k_maplevel_keys", "k_maplevel_accumulate"}, kernels
    assert len(usage) == 3                                                            # k_maplevel_accumulate<MOM> twice
    for k, u in usage.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 64 and u.get("AGPRs", 0) == 0, (k, u)
    src = open(path).read()
    assert len(re.findall(r"__global__", src)) == len(kernels)
    # integer atomics only (the overflow flag; the box and the point total go through map_record_stats), no inline
    # assembly; key codec, insert, sort and selection are called, not copied
    assert re.findall(r"atomic\w*\(", src) == ["atomicAdd("] and "atomicAdd(stats + MS_BAD_COUNT, 1)" in src
    assert not re.search(r"\basm\b", src)
    assert "map_key(" in src and "map_ijk(" in src and "<< 42" not in src
    assert "map_group_batch(" in src and "map_export_order(" in src and "target_from_moments(" in src
