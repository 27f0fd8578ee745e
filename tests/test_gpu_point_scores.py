"""Per-point NDT scores (ndt_score_points), the best voxel and the score-based source filter (ndt_filter_source) on
the GPU, through the Python mirror: the per-point values must add up to what ndt_score_transform reports on the same
handle, agree point by point with the CPU oracle evaluating a one-point source, name a voxel that really is the best of
the point's neighbourhood, line up with the caller's cloud whatever the engine did to its own copy, and leave the
handle's align state alone."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("score", "nearest_voxel_score", "n_neighbors", "best_voxel")

pytestmark = pytest.mark.gpu


def engine(pkg, res, **kw):
    return pkg.NormalDistributionsTransform(device_id=0, resolution=res, step_size=0.1, trans_epsilon=1e-4,
                                            max_iterations=50, **kw)


def methods(pkg, O):
    return ((pkg.DIRECT1, O.DIRECT1), (pkg.DIRECT7, O.DIRECT7), (pkg.DIRECT26, O.DIRECT26), (pkg.KDTREE, O.KDTREE))


def same(a, b):
    return all(a[f].dtype == b[f].dtype and np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)) for f in FIELDS)


def check_sums(ndt, T):
    """Check 1: every point takes part; both sides are f64 and differ in the order of addition only (rel 1e-12, the
    tolerance tests/test_gpu_parity.py uses for re-partitioned sums)."""
    sc = ndt.scoreTransform(T)
    pp = ndt.scorePoints(T)
    nn = pp["n_neighbors"]
    assert len(nn) == ndt.sourceSize()
    assert int(nn.sum(dtype=np.int64)) == sc["n_pairs"]
    assert int((nn > 0).sum()) == sc["n_points_with_neighbors"]
    print("sum(score) %.17g vs %.17g" % (pp["score"].sum(), sc["score"]))
    assert pp["score"].sum() == pytest.approx(sc["score"], rel=1e-12)
    nvtl = pp["nearest_voxel_score"][nn > 0].mean() if (nn > 0).any() else 0.0
    print("nvtl %.17g vs %.17g" % (nvtl, sc["nvtl"]))
    assert nvtl == pytest.approx(sc["nvtl"], rel=1e-12)
    assert np.array_equal(pp["best_voxel"] == -1, pp["nearest_voxel_score"] == 0.0)
    assert np.all(pp["nearest_voxel_score"][nn == 0] == 0.0) and np.all(pp["score"][nn == 0] == 0.0)
    return pp


@pytest.mark.parametrize("name", ["c1", "c2", "c3"])
def test_sums_equal_the_scan_level_call(pkg, O, S, name):
    cfg = {"c1": S.config_c1, "c2": S.config_c2, "c3": S.config_c3}[name]()
    ndt = engine(pkg, cfg["resolution"])
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    aligned = ndt.align(cfg["guess"])
    for fmt in (pkg.RECORDS_F64, pkg.RECORDS_PACKED48):
        ndt.setRecordFormat(fmt)
        for method, _ in methods(pkg, O):
            ndt.setParams(search_method=method)
            for T in (cfg["guess"], aligned):
                check_sums(ndt, T)


def pick_points(pT, res, rng, n_random=512):
    """A seeded random draw plus every point within 1e-3 of a voxel face after the transform."""
    fin = np.isfinite(pT).all(1)
    f = pT.astype(np.float64) / res
    d = np.abs(f - np.round(f)) * res
    near = np.flatnonzero(fin & (d.min(1) < 1e-3))
    rand = rng.choice(len(pT), size=min(n_random, len(pT)), replace=False)
    return np.unique(np.concatenate([near, rand]))


def per_point_case(pkg, O, source, target, T, res, min_points):
    ndt = engine(pkg, res)                                    # the default 80-byte f64 records
    ndt.setInputTarget(target)
    ndt.setInputSource(source)
    kw = dict(resolution=res, step_size=0.1, trans_epsilon=1e-4, max_iterations=50)
    grid = O.Grid(target, O.default_params(**kw))
    OL = grid.export()
    L = ndt.getLeaves()
    assert np.array_equal(L["cell"], OL["cell"])
    rank_of = {int(c): k for k, c in enumerate(L["cell"])}
    d1, d2, _ = O.gauss_constants(res, ndt._p.outlier_ratio)
    pose6 = O.matrix_to_pose(T)
    pT = ndt.transformSource(T)
    sel = pick_points(pT, res, np.random.default_rng(20240607))
    assert len(sel) >= min_points
    src = np.ascontiguousarray(source, np.float32)[:, :3]
    for method, omethod in methods(pkg, O):
        ndt.setParams(search_method=method)
        prm = O.default_params(search_method=omethod, **kw)
        pp = ndt.scorePoints(T)
        worst = [0.0, 0.0, 0.0]
        for i in sel:
            ref = grid.derivatives(src[i:i + 1], pose6, T=T, compute_hessian=False, params=prm)
            # check 2: no exclusions
            assert ref["n_pairs"] == pp["n_neighbors"][i], (method, i)
            assert abs(pp["score"][i] - ref["score"]) <= 1e-9 * abs(ref["score"]) + 1e-12, (method, i)
            assert abs(pp["nearest_voxel_score"][i] - ref["nvtl_sum"]) <= 1e-9 * abs(ref["nvtl_sum"]), (method, i)
            worst[0] = max(worst[0], abs(pp["score"][i] - ref["score"]) / max(abs(ref["score"]), 1e-300))
            # check 3: the best voxel is a member of the oracle's neighbourhood and really is the best of it
            ranks = grid.neighbors(pT[i], omethod)
            cells = [int(OL["cell"][r]) for r in ranks]
            bv, nvs = int(pp["best_voxel"][i]), float(pp["nearest_voxel_score"][i])
            assert (bv == -1) == (nvs == 0.0)
            pair = {}
            for c in set(cells):
                k = rank_of[c]
                x = pT[i].astype(np.float64) - L["mean"][k]
                q = float(x @ L["icov"][k] @ x)
                pair[c] = -d1 * np.exp(-d2 * 0.5 * q) if (q >= -1e-9 and d2 * q * 0.5 <= 50.0) else 0.0
            if bv == -1:
                assert all(v <= 1e-300 for v in pair.values()), (method, i, pair)
                continue
            assert bv in cells, (method, i, bv, cells)
            assert abs(pair[bv] - nvs) <= 1e-9 * nvs, (method, i, pair[bv], nvs)
            assert max(pair.values()) <= nvs * (1 + 1e-9), (method, i)
            worst[1] = max(worst[1], abs(pair[bv] - nvs) / nvs)
        print("method %d: %d points, worst rel score %.3e, worst rel best-voxel recompute %.3e"
              % (method, len(sel), worst[0], worst[1]))


def test_per_point_against_the_oracle_c1(pkg, O, S):
    cfg = S.config_c1()
    per_point_case(pkg, O, cfg["source"], cfg["target"], cfg["guess"], cfg["resolution"], 512)


def test_per_point_against_the_oracle_golden_two_plane(pkg, O, golden_dir):
    z = np.load(os.path.join(golden_dir, "g1_two_plane_3k.npz"))
    per_point_case(pkg, O, z["source"], z["target"], z["guess"], 1.0, 512)


def test_order_views_and_repeats(pkg, S, hipmem):
    cfg = S.config_c2()                                        # 131 072 points: above every sort threshold
    src = np.ascontiguousarray(cfg["source"], np.float32)
    res = cfg["resolution"]
    keep = engine(pkg, res, source_order=pkg.SOURCE_ORDER_KEEP)
    keep.setInputTarget(cfg["target"])
    keep.setInputSource(src)
    T = keep.align(cfg["guess"])
    ref = keep.scorePoints(T)
    assert same(ref, keep.scorePoints(T))                       # two calls in a row
    sort = engine(pkg, res, source_order=pkg.SOURCE_ORDER_SORT)
    sort.setInputTarget(cfg["target"])
    sort.setInputSource(src)
    sort.align(cfg["guess"])                                    # the block-sorted copy exists now
    assert same(ref, sort.scorePoints(T))
    # a viewed device source and a keyframe source
    dx, dy, dz = (hipmem.upload(src[:, k].copy()) for k in range(3))
    keep.setInputSourceDeviceView(dx, dy, dz, len(src))
    assert keep.sourceSize() == len(src) and same(ref, keep.scorePoints(T))
    sort.putKeyframe(7, src)
    sort.setInputSourceFromKeyframe(7)
    assert sort.sourceSize() == len(src) and same(ref, sort.scorePoints(T))
    # a source permuted on the host gives the same values permuted
    perm = np.random.default_rng(5).permutation(len(src))
    keep.setInputSource(src[perm])
    got = keep.scorePoints(T)
    assert same({f: ref[f][perm] for f in FIELDS}, got)
    # the device form writes the same bits
    d = {f: hipmem.upload(np.zeros(len(src), dt)) for f, dt in keep.POINT_SCORE_FIELDS}
    keep.scorePointsDevice(T, d["score"], d["nearest_voxel_score"], d["n_neighbors"], d["best_voxel"], len(src))
    back = {f: np.zeros(len(src), dt) for f, dt in keep.POINT_SCORE_FIELDS}
    for f in FIELDS:
        assert hipmem.rt.hipMemcpy(back[f].ctypes.data, C.c_void_p(d[f]), back[f].nbytes, 2) == 0
    assert same(got, back)


def test_edge_cases(pkg, S):
    cfg = S.config_c1()
    res = cfg["resolution"]
    T = cfg["guess"]
    src = np.ascontiguousarray(cfg["source"], np.float32)
    ndt = engine(pkg, res)
    L = pkg.lib()
    Tc = np.ascontiguousarray(np.asarray(T, np.float32).T).ravel()
    fp = Tc.ctypes.data_as(C.POINTER(C.c_float))
    # no target, no source
    assert L.ndt_score_points(ndt._h, fp, None, None, None, None, 0) == -4        # NDT_ERR_NO_TARGET
    with pytest.raises(pkg.NdtError) as ei:
        ndt.filterSource(T, 0.0)
    assert ei.value.code == -4
    ndt.setInputTarget(cfg["target"])
    assert L.ndt_score_points(ndt._h, fp, None, None, None, None, 0) == -5        # NDT_ERR_NO_SOURCE
    n_out = C.c_size_t(99)
    assert L.ndt_filter_source(ndt._h, fp, 0.0, 0, None, None, 0, C.byref(n_out)) == -5 and n_out.value == 0
    ndt.setInputSource(src)
    ref = ndt.scorePoints(T)
    # NULL outputs in every combination; cap < n with a non-NULL output
    n = len(src)
    for mask in itertools.product((False, True), repeat=4):
        want = [f for f, m in zip(FIELDS, mask) if m]
        got = ndt.scorePoints(T, fields=want)
        assert sorted(got) == sorted(want)
        for f in want:
            assert np.array_equal(got[f], ref[f])
        bufs = [np.zeros(n, dt) if m else None for (f, dt), m in zip(ndt.POINT_SCORE_FIELDS, mask)]
        ptrs = [b.ctypes.data if b is not None else None for b in bufs]
        assert L.ndt_score_points(ndt._h, fp, *ptrs, n - 1) == (-1 if any(mask) else 0)
    # NaN / Inf points report 0 / 0 / 0 / -1 and do not disturb their neighbours in the wave
    bad = src.copy()
    hit = np.array([0, 1, 63, 64, 65, 130, 1000, n - 1])
    bad[hit[0::2], 0] = np.nan
    bad[hit[1::2], 2] = np.inf
    for method in (pkg.DIRECT7, pkg.KDTREE, pkg.DIRECT26, pkg.DIRECT1):
        ndt.setParams(search_method=method)
        ndt.setInputSource(src)
        clean = ndt.scorePoints(T)
        ndt.setInputSource(bad)
        got = check_sums(ndt, T)
        ok = np.ones(n, bool)
        ok[hit] = False
        for f in FIELDS:
            assert np.array_equal(got[f][ok], clean[f][ok])
        assert np.all(got["score"][hit] == 0) and np.all(got["nearest_voxel_score"][hit] == 0)
        assert np.all(got["n_neighbors"][hit] == 0) and np.all(got["best_voxel"][hit] == -1)
        # sizes around a wave and a block
        for m in (1, 63, 64, 65, 257, 1025):
            ndt.setInputSource(src[:m])
            part = check_sums(ndt, T)
            for f in FIELDS:
                assert np.array_equal(part[f], clean[f][:m])
        # a source entirely off the map
        ndt.setInputSource(src + np.float32(1.0e4))
        off = check_sums(ndt, T)
        assert not off["score"].any() and not off["nearest_voxel_score"].any() and not off["n_neighbors"].any()
        assert np.all(off["best_voxel"] == -1)
    # a transform that makes every point non-finite
    Tinf = np.array(T, np.float64)
    Tinf[0, 3] = np.inf
    with pytest.raises(ValueError):
        ndt.scorePoints(Tinf)


def test_multigrid_union_sums(pkg, S):
    cfg = S.config_c1()
    tgt = np.ascontiguousarray(cfg["target"], np.float32)
    ndt = engine(pkg, cfg["resolution"])
    half = len(tgt) // 2
    ndt.addTarget(tgt[:half + 500], 1)                          # overlapping parts: cells shared by both grids
    ndt.addTarget(tgt[half - 500:], 2)
    ndt.createVoxelKdtree()
    ndt.setInputSource(cfg["source"])
    pp = check_sums(ndt, cfg["guess"])
    assert (pp["n_neighbors"] > 0).any()
    assert pp["best_voxel"].max() >= 0 and pp["best_voxel"].min() >= -1


def filter_reference(nvs, thr, below):
    return np.flatnonzero(nvs < thr) if below else np.flatnonzero(nvs >= thr)


def test_filter_matches_the_per_point_values(pkg, S, hipmem):
    cfg = S.config_c2()
    src = np.ascontiguousarray(cfg["source"], np.float32)
    ndt = engine(pkg, cfg["resolution"])
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(src)
    T = ndt.align(cfg["guess"])
    nvs = ndt.scorePoints(T)["nearest_voxel_score"]
    n = len(src)
    ox, oy, oz = (hipmem.upload(np.zeros(n, np.float32)) for _ in range(3))
    oi = hipmem.upload(np.zeros(n, np.int32))
    L = pkg.lib()
    Tc = np.ascontiguousarray(np.asarray(T, np.float32).T).ravel()
    fp = Tc.ctypes.data_as(C.POINTER(C.c_float))

    def download(ptr, m, dt):
        a = np.zeros(m, dt)
        if m:
            assert hipmem.rt.hipMemcpy(a.ctypes.data, C.c_void_p(ptr), a.nbytes, 2) == 0
        return a

    thresholds = [float(np.percentile(nvs[nvs > 0], p)) for p in (10, 50, 90)] + [0.0, float("inf")]
    for thr, below in itertools.product(thresholds, (False, True)):
        want = filter_reference(nvs, thr, below)
        xyz, idx = ndt.filterSource(T, thr, keep_below=below)
        assert np.array_equal(idx, want), (thr, below, len(idx), len(want))
        assert np.array_equal(xyz.view(np.uint32), src[want].view(np.uint32))
        m = ndt.filterSourceDevice(T, thr, below, ox, oy, oz, oi, n)
        assert m == len(want)
        assert np.array_equal(download(oi, m, np.int32), want)
        for k, p in enumerate((ox, oy, oz)):
            assert np.array_equal(download(p, m, np.float32).view(np.uint32), src[want, k].view(np.uint32))
        if len(want):   # cap one short of the result
            with pytest.raises(pkg.NdtError) as ei:
                ndt.filterSourceDevice(T, thr, below, ox, oy, oz, None, len(want) - 1)
            assert ei.value.code == -1 and ndt.last_filter_count == len(want)
            n_out = C.c_size_t(0)
            buf = np.zeros((n, 3), np.float32)
            assert L.ndt_filter_source(ndt._h, fp, thr, int(below), buf.ctypes.data, None, len(want) - 1, C.byref(n_out)) == -1
            assert n_out.value == len(want)
    # the device form's output goes straight into setInputTargetDevice and builds the grid the same points give
    thr = thresholds[1]
    want = filter_reference(nvs, thr, False)
    m = ndt.filterSourceDevice(T, thr, False, ox, oy, oz, None, n)
    a, b = engine(pkg, cfg["resolution"]), engine(pkg, cfg["resolution"])
    a.setInputTargetDevice(ox, oy, oz, m)
    b.setInputTarget(src[want])
    La, Lb = a.getLeaves(), b.getLeaves()
    for k in ("cell", "count", "mean", "icov"):
        assert np.array_equal(La[k], Lb[k]), k
    # the handle's own source is unchanged
    assert np.array_equal(ndt.scorePoints(T)["nearest_voxel_score"], nvs)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1024 * 256 + 1, 1000003])
def test_filter_sizes_around_a_wave_a_block_and_a_million(pkg, S, n):
    cfg = S.config_c1()
    base = np.ascontiguousarray(cfg["source"], np.float32)
    rng = np.random.default_rng(n)
    src = base[rng.integers(0, len(base), size=n)] + rng.normal(0, 0.05, size=(n, 3)).astype(np.float32)
    ndt = engine(pkg, cfg["resolution"])
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(src)
    T = cfg["guess"]
    nvs = check_sums(ndt, T)["nearest_voxel_score"]
    thr = float(np.median(nvs))
    for below in (False, True):
        want = filter_reference(nvs, thr, below)
        xyz, idx = ndt.filterSource(T, thr, keep_below=below)
        assert np.array_equal(idx, want)
        assert np.array_equal(xyz.view(np.uint32), src[want].view(np.uint32))


def test_nothing_else_moved(pkg, S):
    cfg = S.config_c2()
    ndt = engine(pkg, cfg["resolution"])
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])

    def align_bits():
        ndt.align(cfg["guess"])
        r = ndt._raw
        return bytes(bytearray(r.final_transformation)) + bytes(bytearray(r.hessian)) + np.float64(r.score).tobytes(), r.iterations

    before, iters = align_bits()
    hist = ndt.getIterationHistory()
    launches = ndt.getTiming()["n_eval_launches"]
    T = ndt.getFinalTransformation()
    ndt.scorePoints(T)
    ndt.filterSource(T, 0.5)
    ndt.filterSource(T, 0.5, keep_below=True)
    assert ndt.getTiming()["n_eval_launches"] == launches
    after_hist = ndt.getIterationHistory()
    assert len(after_hist[1]) == iters + 1
    for a, b in zip(hist, after_hist):
        assert np.array_equal(a, b)
    assert np.array_equal(ndt.getFinalTransformation(), T)
    again, iters2 = align_bits()
    assert again == before and iters2 == iters


def test_cpp_adapter_agrees_with_the_c_calls():
    """tests/cpp/test_point_scores.cpp, built with the g++ line of tests/cpp/Makefile."""
    d = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(d, "test_point_scores")
    lib = os.path.join(ROOT, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include", "compat"),
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(d, "test_point_scores.cpp"), lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "point scores: OK" in p.stdout
