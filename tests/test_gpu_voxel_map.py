"""The sparse voxel map (ndt_map_*): accumulated scan by scan it exports, bit for bit, what pcl::VoxelGrid gives for the
concatenation of everything added -- against (A) voxelDownsample on the concatenated cloud where its dense index allows
it, and (B) a NumPy restatement: int64 voxel coordinates from f32 floor(p * inv), a stable lexicographic (k, j, i) sort,
f32 sums per voxel in input order.  Every comparison is np.array_equal on the bits: both sides do the same f32
operations in the same order."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def host_transform_f64(T, pts):
    """pcl::transformPointCloud with a double matrix: f64 products summed left to right, one rounding to f32."""
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    out = np.empty((len(pts), 3), np.float32)
    for r in range(3):
        out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
    return out


def voxel_ijk(pts, leaf):
    inv = np.float32(1.0) / np.float32(leaf)
    return np.floor(np.asarray(pts, np.float32)[:, :3] * inv).astype(np.int64)


def voxelmap_numpy(pts, leaf, intensity=None):
    """Yardstick (B): (centroids [m,3] f32, intensity [m] f32 or None, counts [m] int32, ijk [m,3] int64), ascending
    (k, j, i); no dense index, no bounding box."""
    p = np.asarray(pts, np.float32)[:, :3]
    fin = np.isfinite(p).all(axis=1)
    q = p[fin]
    ijk = voxel_ijk(q, leaf)
    order = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))          # stable; the last key is the primary one
    s = ijk[order]
    heads = np.nonzero(np.r_[True, (s[1:] != s[:-1]).any(axis=1)])[0]
    counts = np.diff(np.r_[heads, len(s)])
    cols = [q[order, 0], q[order, 1], q[order, 2]]
    if intensity is not None:
        cols.append(np.asarray(intensity, np.float32)[fin][order])
    sums = [np.zeros(len(heads), np.float32) for _ in cols]
    for j in range(int(counts.max())):                             # sequential float sums, vectorised over the voxels
        live = counts > j
        for acc, c in zip(sums, cols):
            acc[live] = acc[live] + c[heads[live] + j]
    nf = counts.astype(np.float32)
    out = [acc / nf for acc in sums]
    return np.stack(out[:3], axis=1), (out[3] if intensity is not None else None), counts.astype(np.int32), s[heads]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def engine(pkg, **kw):
    return pkg.NormalDistributionsTransform(device_id=0, **kw)


def export_bits(ndt, inten=False, min_points=1):
    out, cnt = ndt.mapExport(min_points=min_points, columns=5 if inten else 3, intensity_column=4 if inten else None,
                             with_counts=True)
    return bits(out).copy(), cnt.copy()


def assert_equals_b(ndt, pts, leaf, intensity=None, min_points=1):
    xyz, inten, counts, _ = voxelmap_numpy(pts, leaf, intensity)
    keep = counts >= min_points
    out, cnt = ndt.mapExport(min_points=min_points, columns=5 if intensity is not None else 3,
                             intensity_column=4 if intensity is not None else None, with_counts=True)
    assert len(out) == int(keep.sum())
    assert same(out[:, :3], xyz[keep])
    assert np.array_equal(cnt, counts[keep])
    if intensity is not None:
        assert same(out[:, 4], inten[keep])
    return out, cnt


@pytest.fixture(scope="module")
def stream6():
    from slam_sam_amd import replay
    return replay.make_stream(n_frames=6, beams=64, cols=512)


def test_equal_to_the_batch_filter(pkg, stream6):
    leaf = 0.5
    rng = np.random.default_rng(11)
    ndt = engine(pkg)
    ndt.mapReset(leaf, with_intensity=True)
    moved = []
    for scan, T in stream6:
        cloud = np.zeros((len(scan), 5), np.float32)
        cloud[:, :3] = scan[:, :3]
        cloud[:, 4] = rng.uniform(0, 255, len(scan)).astype(np.float32)
        ndt.mapAdd(cloud, intensity_column=4, pose=T)
        m = cloud.copy()
        m[:, :3] = host_transform_f64(T, scan)
        moved.append(m)
    cat = np.concatenate(moved)
    out, cnt = assert_equals_b(ndt, cat, leaf, cat[:, 4])                     # (B)
    batch = ndt.voxelDownsample(cat, leaf, intensity_column=4)                # (A): the dense-index filter on the concatenation
    assert same(out[:, :3], batch[:, :3]) and same(out[:, 4], batch[:, 4])
    info = ndt.mapInfo()
    fin = np.isfinite(cat[:, :3]).all(axis=1)
    ijk = voxel_ijk(cat[fin], leaf)
    assert info["n_voxels"] == len(out) and info["n_points"] == int(fin.sum()) == int(cnt.sum())
    assert info["n_points_dropped"] == int((~fin).sum()) and info["n_adds"] == 6
    assert info["min_ijk"] == tuple(ijk.min(0)) and info["max_ijk"] == tuple(ijk.max(0))
    assert info["with_intensity"] and info["leaf"] == np.float32(leaf) and info["capacity"] >= 2 * info["n_voxels"]


def test_splitting_does_not_matter(pkg):
    leaf = 0.5
    rng = np.random.default_rng(3)
    cloud = rng.uniform([-5, -5, -1], [5, 5, 1], (20000, 3)).astype(np.float32)
    sizes = [1, 63, 64, 65, 257, 4097]
    cuts = np.r_[0, np.cumsum(sizes), len(cloud)]
    piece = np.repeat(np.arange(len(cuts) - 1), np.diff(cuts))
    # a voxel that receives points from three or more pieces, and two or more from one of them
    ijk = voxel_ijk(cloud, leaf)
    _, vox = np.unique(ijk, axis=0, return_inverse=True)
    vox = vox.ravel()
    pairs = np.unique(np.stack([vox, piece], axis=1), axis=0)
    pieces_per_voxel = np.bincount(pairs[:, 0])
    busy = np.nonzero(pieces_per_voxel >= 3)[0]
    assert len(busy) > 0
    assert any(np.bincount(piece[vox == v]).max() >= 2 for v in busy[:50])

    def run(split):
        ndt = engine(pkg)
        ndt.mapReset(leaf)
        if split:
            for a, b in zip(cuts[:-1], cuts[1:]):
                ndt.mapAdd(cloud[a:b])
        else:
            ndt.mapAdd(cloud)
        return export_bits(ndt)

    whole, whole_cnt = run(False)
    for _ in range(2):                                                       # the same sequence twice: identical bits
        split, split_cnt = run(True)
        assert np.array_equal(split, whole) and np.array_equal(split_cnt, whole_cnt)
    xyz, _, counts, _ = voxelmap_numpy(cloud, leaf)
    assert np.array_equal(whole, bits(xyz)) and np.array_equal(whole_cnt, counts)


def test_growth_and_collisions(pkg):
    leaf = 0.5
    rng = np.random.default_rng(5)
    cloud = rng.uniform([-30, -30, -3], [30, 30, 3], (24000, 3)).astype(np.float32)
    cuts = [0, 200, 1000, 4000, 12000, 24000]
    small, big = engine(pkg), engine(pkg)
    small.mapReset(leaf, initial_capacity=64)
    big.mapReset(leaf)
    assert small.mapInfo()["capacity"] == 64
    for a, b in zip(cuts[:-1], cuts[1:]):
        small.mapAdd(cloud[a:b])
        big.mapAdd(cloud[a:b])
        info = small.mapInfo()
        assert info["capacity"] >= 2 * info["n_voxels"]
    info = small.mapInfo()
    assert info["n_voxels"] >= 5000 and info["n_grows"] >= 3
    assert info["capacity"] >= 2 * info["n_voxels"] and info["capacity"] & (info["capacity"] - 1) == 0
    assert big.mapInfo()["n_grows"] == 0 and big.mapInfo()["n_voxels"] == info["n_voxels"]
    out, cnt = assert_equals_b(small, cloud, leaf)
    b_out, b_cnt = export_bits(big)
    assert np.array_equal(bits(out), b_out) and np.array_equal(cnt, b_cnt)


def test_one_crowded_voxel_and_the_edges_of_the_index(pkg):
    leaf = 0.5                       # inv_leaf = 2 exactly, so every arithmetic agrees on a face; inexact leaves: test_gpu_map_sweep.py
    rng = np.random.default_rng(7)
    crowd = rng.uniform([-0.5, -0.5, -0.5], [-0.001, -0.001, -0.001], (5000, 3)).astype(np.float32)   # voxel (-1, -1, -1)
    around = rng.uniform([-6, -6, -2], [6, 6, 2], (400, 3)).astype(np.float32)
    g = np.array([-1.0, -0.5, -0.0, 0.0, 0.5, 1.0], np.float32)
    faces = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)    # on voxel faces, -0.0 included
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [1, -np.inf, np.nan]], np.float32)
    cloud = np.concatenate([crowd[:2000], bad[:2], around, faces, bad[2:], crowd[2000:], faces[::-1]])
    perm = np.random.default_rng(8).permutation(len(cloud))
    cloud = np.ascontiguousarray(cloud[perm])
    # floor, not truncation: -0.25 is in voxel -1, and -0.0 in voxel 0
    assert voxel_ijk(np.array([[-0.25, -0.0, 0.5]], np.float32), leaf).tolist() == [[-1, 0, 1]]
    ndt = engine(pkg)
    ndt.mapReset(leaf)
    half = len(cloud) // 2
    ndt.mapAdd(cloud[:half])
    ndt.mapAdd(cloud[half:])
    info = ndt.mapInfo()
    assert info["n_points_dropped"] == len(bad) and info["n_points"] == len(cloud) - len(bad)
    out, cnt = assert_equals_b(ndt, cloud, leaf)
    assert cnt.max() >= 5000
    assert info["min_ijk"] == tuple(voxel_ijk(cloud[np.isfinite(cloud).all(1)], leaf).min(0))


def test_where_the_dense_filter_refuses(pkg):
    leaf = 0.1
    rng = np.random.default_rng(9)
    a = rng.uniform([-20, -20, -5], [20, 20, 5], (3000, 3)).astype(np.float32)
    b = rng.uniform([29980, -20, -5], [30020, 20, 5], (3000, 3)).astype(np.float32)
    cat = np.concatenate([a, b])
    ijk = voxel_ijk(cat, leaf)
    ext = ijk.max(0) - ijk.min(0) + 1
    assert int(ext[0]) * int(ext[1]) * int(ext[2]) > 2**31 - 1               # about 1.2e10 cells
    assert np.floor(np.float32(30040.0) * (np.float32(1.0) / np.float32(leaf))) < 2**20 and np.abs(ijk).max() < 2**20
    ndt = engine(pkg)
    with pytest.raises(pkg.NdtError) as ei:
        ndt.voxelDownsample(cat, leaf)
    assert ei.value.code == -6                                               # NDT_ERR_GRID_OVERFLOW
    ndt.mapReset(leaf)
    ndt.mapAdd(a)
    ndt.mapAdd(b)
    assert_equals_b(ndt, cat, leaf)


def test_refusals_leave_the_map_as_it_was(pkg, hipmem):
    leaf = 0.5
    rng = np.random.default_rng(13)
    ndt = engine(pkg)
    cloud = np.zeros((6000, 5), np.float32)
    cloud[:, :3] = rng.uniform([-10, -10, -2], [10, 10, 2], (6000, 3))
    cloud[:, 4] = rng.uniform(0, 255, 6000)

    def refused(code, call):
        with pytest.raises(pkg.NdtError) as ei:
            call()
        assert ei.value.code == code
        return str(ei.value)

    no_map_calls = (ndt.mapInfo, lambda: ndt.mapAdd(cloud), ndt.mapExport, ndt.setInputTargetFromMap,
                    lambda: ndt.mapAddKeyframe(1, np.eye(4)), lambda: ndt.mapExportDevice(0, 0, 0, 0),
                    lambda: ndt.mapAddDevice(0, 0, 0, 0))
    for call in no_map_calls:                                                # before mapReset
        refused(-1, call)
    ndt.mapReset(leaf, with_intensity=True)
    ndt.mapAdd(cloud, intensity_column=4)
    kept, kept_cnt = export_bits(ndt, inten=True)
    info = ndt.mapInfo()

    def unchanged():
        now, now_cnt = export_bits(ndt, inten=True)
        assert np.array_equal(now, kept) and np.array_equal(now_cnt, kept_cnt)
        assert ndt.mapInfo() == info

    far = cloud[:100].copy()
    far[37, 0] = np.float32(2**20 * leaf)                                    # one finite point at the limit
    refused(-6, lambda: ndt.mapAdd(far, intensity_column=4))
    unchanged()
    far[37, 0] = np.float32(-3.0e30)
    refused(-6, lambda: ndt.mapAdd(far, intensity_column=4))
    unchanged()
    refused(-1, lambda: ndt.mapAdd(cloud[:100]))                             # a with-intensity map, a cloud without
    unchanged()
    ndt.putKeyframe(1, cloud[:100, :3])
    refused(-1, lambda: ndt.mapAddKeyframe(1, np.eye(4)))                    # the archive keeps xyz only
    unchanged()
    d = [hipmem.upload(np.ascontiguousarray(cloud[:100, k])) for k in range(3)]
    refused(-1, lambda: ndt.mapAddDevice(d[0], d[1], d[2], 100))             # d_intensity == NULL
    unchanged()
    o = [hipmem.upload(np.zeros(10, np.float32)) for _ in range(3)]
    msg = refused(-1, lambda: ndt.mapExportDevice(o[0], o[1], o[2], 10))     # too small a cap: the needed size is named
    assert str(info["n_voxels"]) in msg
    unchanged()
    ndt.mapAdd(cloud[:0], intensity_column=4)                                # n = 0: a no-op
    unchanged()
    # a point just inside the limit is taken
    edge = engine(pkg)
    edge.mapReset(leaf)
    inside = np.array([[2**20 * leaf - 0.25, 0, 0], [-(2**20) * leaf + 0.5, 0, 0]], np.float32)    # voxels 2^20 - 1 and -(2^20 - 1)
    edge.mapAdd(inside)
    assert edge.mapInfo()["max_ijk"][0] == 2**20 - 1 and edge.mapInfo()["min_ijk"][0] == -(2**20) + 1
    assert_equals_b(edge, inside, leaf)
    refused(-6, lambda: edge.mapAdd(np.array([[-(2**20) * leaf + 0.25, 0, 0]], np.float32)))       # floor: voxel -2^20
    assert_equals_b(edge, inside, leaf)
    ndt.mapClear()
    for call in no_map_calls:                                                # after mapClear
        refused(-1, call)


def test_min_points(pkg):
    leaf = 0.5
    rng = np.random.default_rng(17)
    cloud = rng.uniform([-8, -8, -1], [8, 8, 1], (9000, 3)).astype(np.float32)
    ndt = engine(pkg)
    ndt.mapReset(leaf)
    ndt.mapAdd(cloud[:5000])
    ndt.mapAdd(cloud[5000:])
    _, cnt = assert_equals_b(ndt, cloud, leaf, min_points=3)
    assert cnt.min() >= 3 and len(cnt) < ndt.mapInfo()["n_voxels"]
    all_cnt = voxelmap_numpy(cloud, leaf)[2]
    out, cnt = ndt.mapExport(min_points=int(all_cnt.max()) + 1, with_counts=True)     # above every count: empty, NDT_OK
    assert out.shape == (0, 3) and len(cnt) == 0
    with pytest.raises(pkg.NdtError) as ei:
        ndt.setInputTargetFromMap(int(all_cnt.max()) + 1)
    assert ei.value.code == -4                                               # NDT_ERR_NO_TARGET
    assert_equals_b(ndt, cloud, leaf)                                        # the map is as it was


@pytest.mark.parametrize("capacity", [1 << 20, 1 << 21])
def test_export_at_the_scan_pass_boundary(pkg, capacity):
    """The export's block offsets come from the engine's one-block scan, 1024 block counts per pass: a table of 2^20
    slots is 1024 export blocks (exactly one pass), one of 2^21 is 2048 (two passes, the second behind the first's
    carry).  The hash spreads a few thousand voxels over the whole table."""
    leaf = 0.5
    rng = np.random.default_rng(23)
    cloud = rng.uniform([-8, -8, -1], [8, 8, 1], (3000, 3)).astype(np.float32)
    counts = voxelmap_numpy(cloud, leaf)[2]
    assert (counts == 1).sum() > 100 and (counts >= 2).sum() > 100
    ndt = engine(pkg)
    ndt.mapReset(leaf, initial_capacity=capacity)
    assert ndt.mapInfo()["capacity"] == capacity
    ndt.mapAdd(cloud[:1700])
    ndt.mapAdd(cloud[1700:])
    assert ndt.mapInfo()["capacity"] == capacity and ndt.mapInfo()["n_grows"] == 0
    assert_equals_b(ndt, cloud, leaf, min_points=1)
    assert_equals_b(ndt, cloud, leaf, min_points=2)


def test_keyframes_and_the_target(pkg, stream6, hipmem):
    leaf = 0.5
    kw = dict(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=35)
    ndt = engine(pkg, **kw)
    ndt.mapReset(leaf)
    for k, (scan, T) in enumerate(stream6[:5]):
        ndt.putKeyframe(100 + k, scan)
    for k, (scan, T) in enumerate(stream6[:5]):
        ndt.mapAddKeyframe(100 + k, T)
    host = np.concatenate([host_transform_f64(T, scan) for scan, T in stream6[:5]])
    out, _ = assert_equals_b(ndt, host, leaf)
    ndt.setInputTargetFromMap(1)
    from_map = ndt.getLeaves()
    assert ndt.getGridInfo()["n_target_points"] == len(out) and len(from_map["cell"]) > 100
    ref = engine(pkg, **kw)
    ref.setInputTarget(out)                                                  # the host copy of the export
    want = ref.getLeaves()
    for f in ("cell", "count", "mean", "cov", "icov"):
        assert np.array_equal(from_map[f], want[f]), f
    n = ndt.mapInfo()["n_voxels"]
    o = [hipmem.upload(np.zeros(n, np.float32)) for _ in range(3)]
    oc = hipmem.upload(np.zeros(n, np.int32))
    assert ndt.mapExportDevice(o[0], o[1], o[2], n, o_count=oc) == n
    dev = engine(pkg, **kw)
    dev.setInputTargetDevice(o[0], o[1], o[2], n)
    got = dev.getLeaves()
    for f in ("cell", "count", "mean", "cov", "icov"):
        assert np.array_equal(got[f], want[f]), f
    back = np.zeros(n, np.int32)
    assert hipmem.rt.hipMemcpy(back.ctypes.data, C.c_void_p(oc), back.nbytes, 2) == 0
    assert np.array_equal(back, voxelmap_numpy(host, leaf)[2])
    assert ndt.keyframeCount() == 5                                          # the archive is as it was


def test_the_handle_is_untouched(pkg, S):
    cfg = S.config_c2()
    ndt = engine(pkg, resolution=cfg["resolution"], step_size=0.1, trans_epsilon=1e-4, max_iterations=35)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])

    def align_bits():
        ndt.align(cfg["guess"])
        r = ndt._raw
        return bytes(bytearray(r.final_transformation)) + bytes(bytearray(r.hessian)) + np.float64(r.score).tobytes(), r.iterations

    before, iters = align_bits()
    hist = ndt.getIterationHistory()
    launches = ndt.getTiming()["n_eval_launches"]
    leaves = ndt.getLeaves()
    ndt.mapReset(0.5, initial_capacity=64)
    ndt.mapAdd(cfg["source"][:, :3], pose=cfg["guess"])
    ndt.mapAdd(cfg["target"][:20000, :3])
    assert len(ndt.mapExport()) == ndt.mapInfo()["n_voxels"] > 0
    ndt.mapClear()
    after = ndt.getLeaves()
    for f in leaves:
        assert np.array_equal(leaves[f], after[f]), f
    assert ndt.getTiming()["n_eval_launches"] == launches
    for a, b in zip(hist, ndt.getIterationHistory()):
        assert np.array_equal(a, b)
    again, iters2 = align_bits()
    assert again == before and iters2 == iters


def test_cpp_adapter(pkg):
    """tests/cpp/test_voxel_map.cpp against the API mocks, built with the g++ line tests/cpp/Makefile uses for them."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "tests", "cpp")
    exe = os.path.join(d, "test_voxel_map")
    lib = os.path.join(root, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(root, "include", "compat"), "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(d, "test_voxel_map.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "voxel map: PASS" in p.stdout
