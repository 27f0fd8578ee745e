"""The host-cloud boundary (ndt_host_cloud.h, upload_column / download_strided): every host form that takes a
strided cloud gives, bit for bit, what its device form gives for the same columns, whatever the layout -- 3 columns, 4 with
the intensity in column 3, 8 with it in column 7 or 4, the other columns filled with junk --; every host form that writes
a cloud writes x, y, z and the intensity field of the first m points and nothing else (the output is pre-filled with a
sentinel bit pattern); and the three capacity behaviours: ndt_map_export writes what fits and then reports the total,
a compaction's download is refused with nothing written, ndt_voxel_downsample is refused inside its device form."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYOUTS = [(3, None), (4, 3), (8, 7), (8, 4)]            # (columns, intensity column)
SIZES = [0, 1, 65, 3000]
SENTINEL = np.uint32(0xFFC5A5A5)                         # (a NaN with a payload no computation produces)
INVALID_ARG = -1


@pytest.fixture(scope="module")
def ndt(pkg):
    e = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0, min_points_per_voxel=3)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_cloud(n, cols, icol, seed, nan_every=0):
    """(the cloud [n, cols] with junk in the columns nobody owns, xyz [n, 3], intensity [n])"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1e6, 1e6, (n, cols)).astype(np.float32)
    xyz = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    if nan_every and n > 1:
        xyz[::nan_every, 0] = np.nan
    inten = rng.uniform(0.0, 255.0, n).astype(np.float32)
    a[:, :3] = xyz
    if icol is not None:
        a[:, icol] = inten
    return a, xyz, inten


def stride_off(a, cols, icol):
    return 4 * cols, -1 if icol is None else 4 * icol


def upload_columns(hipmem, xyz, inten=None):
    d = [hipmem.upload(xyz[:, k].copy()) for k in range(3)]
    return d + [None if inten is None else hipmem.upload(inten)]


def device_out(hipmem, n, k=4, dtype=np.float32):
    return [hipmem.upload(np.zeros(max(n, 1), dtype)) for _ in range(k)]


def download(hipmem, ptr, n, dtype=np.float32):
    out = np.zeros(n, dtype)
    if n:
        assert hipmem.rt.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return out


def sentinel_cloud(rows, cols):
    return np.full((rows, cols), SENTINEL, np.uint32).view(np.float32)


def check_written(out, m, cols, icol, xyz, inten, what=""):
    """rows [0, m): x, y, z (and the intensity) as given, every other column the sentinel; rows from m on: untouched"""
    b = bits(out)
    assert np.array_equal(b[:m, :3], bits(xyz)[:m]), what
    owned = [0, 1, 2]
    if icol is not None:
        assert np.array_equal(b[:m, icol], bits(inten)[:m]), what
        owned.append(icol)
    rest = [c for c in range(cols) if c not in owned]
    assert np.all(b[:m, rest] == SENTINEL), what
    assert np.all(b[m:] == SENTINEL), what


def last_error(pkg, ndt):
    return pkg.lib().ndt_last_error(ndt._h).decode()


def state_equal(s0, s1):
    return all(np.array_equal(bits(s0[k]), bits(s1[k])) for k in ("ijk", "count", "sums"))


# ---- host forms that take a cloud ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cols,icol", LAYOUTS)
def test_map_add_and_keyframe(pkg, ndt, hipmem, cols, icol, n):
    a, xyz, inten = make_cloud(n, cols, icol, 11 + n)
    d = upload_columns(hipmem, xyz, inten if icol is not None else None)
    pose = np.eye(4)
    pose[:3, 3] = [0.25, -1.5, 2.0]
    ndt.mapReset(0.5, with_intensity=icol is not None)
    ndt.mapAddDevice(d[0], d[1], d[2], n, d_intensity=d[3], pose=pose)
    want = ndt.mapExportState()
    assert len(want["count"]) > 0 or n == 0
    ndt.mapReset(0.5, with_intensity=icol is not None)
    ndt.mapAdd(a, intensity_column=icol, pose=pose)        # (n = 0: accepted, nothing is uploaded)
    assert state_equal(ndt.mapExportState(), want)
    # the keyframe archive holds xyz only: against the device add of the same columns
    ndt.mapReset(0.5)
    ndt.mapAddDevice(d[0], d[1], d[2], n, pose=pose)
    want = ndt.mapExportState()
    ndt.mapReset(0.5)
    ndt.putKeyframe(77, a)                                 # (n = 0: accepted, the stride is still checked)
    ndt.mapAddKeyframe(77, pose)
    assert state_equal(ndt.mapExportState(), want)
    ndt.eraseKeyframe(77)
    ndt.mapClear()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cols,icol", LAYOUTS)
def test_map_carve_label_points_and_scan_context(pkg, ndt, hipmem, cols, icol, n):
    a, xyz, _ = make_cloud(n, cols, icol, 23 + n)
    d = upload_columns(hipmem, xyz)
    world, _, _ = make_cloud(3000, 3, None, 5)
    w = upload_columns(hipmem, world)
    origin = [0.1, 0.2, 0.3]
    got = []
    for host in (False, True):
        ndt.mapReset(0.5)
        ndt.mapAddDevice(w[0], w[1], w[2], len(world))
        if host:
            r = ndt.mapCarve(a, origin, min_misses=1, keep_last=0)
            labels, k = pkg.mapLabelPoints(ndt, a)
        else:
            r = ndt.mapCarveDevice(d[0], d[1], d[2], n, origin, min_misses=1, keep_last=0)
            d_label = hipmem.upload(np.full(max(n, 1), -7, np.int32))
            k = pkg.mapLabelPointsDevice(ndt, d[0], d[1], d[2], n, d_label)
            labels = download(hipmem, d_label, n, np.int32)
        got.append((r, ndt.mapExportState(), labels, k))
    assert got[0][0] == got[1][0] and state_equal(got[0][1], got[1][1])
    assert n == 0 or got[0][0]["n_rays"] > 0
    assert np.array_equal(got[0][2], got[1][2]) and got[0][3] == got[1][3]
    ndt.mapClear()
    desc, count = pkg.scanContext(ndt, a, with_count=True)
    R, S = desc.shape
    d_desc, d_count = hipmem.upload(np.zeros(R * S, np.float32)), hipmem.upload(np.zeros(R * S, np.int32))
    pkg.scanContextDevice(ndt, d[0], d[1], d[2], n, d_desc, d_count)
    assert np.array_equal(bits(desc).ravel(), bits(download(hipmem, d_desc, R * S)))
    assert np.array_equal(count.ravel(), download(hipmem, d_count, R * S, np.int32))
    assert n < 3000 or count.sum() > 0


@pytest.mark.parametrize("n", SIZES[1:])                   # (ndt_multigrid_add_target refuses n = 0: below)
@pytest.mark.parametrize("cols,icol", LAYOUTS)
def test_multigrid_add_target(pkg, hipmem, cols, icol, n):
    """there is no device form: a union of one grid against the single grid built from the same columns on the device"""
    a, xyz, _ = make_cloud(n, cols, icol, 31 + n)
    d = upload_columns(hipmem, xyz)
    kw = dict(device_id=0, resolution=8.0, min_points_per_voxel=3)
    ref = pkg.NormalDistributionsTransform(search_method=pkg.KDTREE, **kw)
    e = pkg.NormalDistributionsTransform(**kw)
    try:
        ref.setInputTargetDevice(d[0], d[1], d[2], n)
        want = ref.getLeaves()
        with pytest.raises(pkg.NdtError) as ei:              # n = 0 is refused, whatever the layout
            e.addTarget(a[:0], 4)
        assert ei.value.code == INVALID_ARG and e.targetCount() == 0
        e.addTarget(a, 3)
        assert (len(want["count"]) > 0) == (n > 1)          # (n = 1: no voxel holds three points)
        if n == 1:
            with pytest.raises(pkg.NdtError):
                e.createVoxelKdtree()
            return
        e.createVoxelKdtree()
        got = e.getLeaves()
        for f in ("count", "mean", "cov", "icov"):
            assert np.array_equal(got[f], want[f]), f
    finally:
        ref.close()
        e.close()


def downsample_host(pkg, ndt, a, cols, icol, leaf, out, cap):
    stride, off = stride_off(a, cols, icol)
    m = C.c_size_t(0)
    rc = pkg.lib().ndt_voxel_downsample(ndt._h, a.ctypes.data, len(a), stride, off, float(leaf), out.ctypes.data, cap, C.byref(m))
    return rc, int(m.value)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cols,icol", LAYOUTS)
def test_voxel_downsample(pkg, ndt, hipmem, cols, icol, n):
    a, xyz, inten = make_cloud(n, cols, icol, 41 + n, nan_every=9)
    d = upload_columns(hipmem, xyz, inten if icol is not None else None)
    o = device_out(hipmem, n)
    total = ndt.voxelDownsampleDevice(d[0], d[1], d[2], n, 1.0, o[0], o[1], o[2], n, d_intensity=d[3],
                                      o_intensity=o[3] if icol is not None else None)
    assert (total > 0) == (n > 0) and (n < 3000 or total < n)
    want = np.stack([download(hipmem, o[k], total) for k in range(3)], axis=1)
    want_i = download(hipmem, o[3], total)
    out = sentinel_cloud(n + 2, cols)
    rc, m = downsample_host(pkg, ndt, a, cols, icol, 1.0, out, n)
    assert rc == 0 and m == total
    check_written(out, m, cols, icol, want, want_i)
    assert total > 1 or n <= 1                              # (the capacity case below runs for n = 65 and n = 3000)
    if total > 1:   # one voxel too few: refused inside the device form with the size that is needed, nothing is written
        out = sentinel_cloud(n + 2, cols)
        rc, m = downsample_host(pkg, ndt, a, cols, icol, 1.0, out, total - 1)
        assert rc == INVALID_ARG and m == total and ("%d occupied voxels" % total) in last_error(pkg, ndt)
        assert np.all(bits(out) == SENTINEL)


KNOT_T = np.array([0.0, 1.0])


def knot_poses():
    kp = np.stack([np.eye(4), np.eye(4)])
    c, s = np.cos(0.3), np.sin(0.3)
    kp[1, :3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    kp[1, :3, 3] = [1.0, -2.0, 0.5]
    return kp


def deskew_host(pkg, ndt, a, cols, icol, t, filt, out, idx, cap):
    kt, poses, nk, _ = pkg._trajectory_args(KNOT_T, knot_poses(), None)
    stride, off = stride_off(a, cols, icol)
    m = C.c_size_t(0)
    rc = pkg.lib().ndt_deskew(ndt._h, a.ctypes.data, len(a), stride, off, t.ctypes.data, pkg._dp(kt), pkg._dp(poses), nk, None,
                              ndt._filter_ref(filt), out.ctypes.data, idx.ctypes.data, cap, C.byref(m))
    return rc, int(m.value)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cols,icol", LAYOUTS)
def test_deskew(pkg, ndt, hipmem, cols, icol, n, compact):
    a, xyz, inten = make_cloud(n, cols, icol, 53 + n, nan_every=7)
    t = np.random.default_rng(n).uniform(-0.1, 1.1, n).astype(np.float32)
    filt = pkg.ScanFilter() if compact else None            # (the zeroed filter drops the non-finite points)
    d = upload_columns(hipmem, xyz, inten if icol is not None else None)
    o = device_out(hipmem, n)
    d_t, d_idx = hipmem.upload(t), hipmem.upload(np.zeros(max(n, 1), np.int32))
    m_dev = ndt.deskewDevice(d[0], d[1], d[2], d_t, n, KNOT_T, knot_poses(), o[0], o[1], o[2], n, filter=filt, d_intensity=d[3],
                             o_intensity=o[3] if icol is not None else None, d_index=d_idx)
    assert m_dev == (np.isfinite(xyz).all(axis=1).sum() if compact else n)
    want = np.stack([download(hipmem, o[k], m_dev) for k in range(3)], axis=1)
    want_i, want_idx = download(hipmem, o[3], m_dev), download(hipmem, d_idx, m_dev, np.int32)
    out, idx = sentinel_cloud(n + 2, cols), np.full(n + 2, -9, np.int32)
    rc, m = deskew_host(pkg, ndt, a, cols, icol, t, filt, out, idx, n)
    assert rc == 0 and m == m_dev
    check_written(out, m, cols, icol, want, want_i)
    assert np.array_equal(idx[:m], want_idx) and np.all(idx[m:] == -9)
    assert m_dev > 1 or n <= 1
    if compact and m_dev > 1:   # a selection the output does not hold: refused behind the launches, nothing is written
        out, idx = sentinel_cloud(n + 2, cols), np.full(n + 2, -9, np.int32)
        rc, m = deskew_host(pkg, ndt, a, cols, icol, t, filt, out, idx, m_dev - 1)
        assert rc == INVALID_ARG and ("%d points selected" % m_dev) in last_error(pkg, ndt)
        assert np.all(bits(out) == SENTINEL) and np.all(idx == -9)


# ---- host forms that only write a cloud ------------------------------------------------------------------------------------
def map_export_host(pkg, ndt, cols, icol, out, cnt, cap):
    m = C.c_size_t(0)
    rc = pkg.lib().ndt_map_export(ndt._h, 1, out.ctypes.data, 4 * cols, -1 if icol is None else 4 * icol, cnt.ctypes.data, cap,
                                  C.byref(m))
    return rc, int(m.value)


@pytest.mark.parametrize("n", SIZES[1:])
@pytest.mark.parametrize("cols,icol", LAYOUTS)
def test_map_export(pkg, ndt, hipmem, cols, icol, n):
    _, xyz, inten = make_cloud(n, 3, None, 61 + n)
    d = upload_columns(hipmem, xyz, inten if icol is not None else None)
    ndt.mapReset(1.0, with_intensity=icol is not None)
    ndt.mapAddDevice(d[0], d[1], d[2], n, d_intensity=d[3])
    total = ndt.mapInfo()["n_voxels"]
    o, o_cnt = device_out(hipmem, total), hipmem.upload(np.zeros(total, np.int32))
    assert ndt.mapExportDevice(o[0], o[1], o[2], total, o_intensity=o[3] if icol is not None else None, o_count=o_cnt) == total
    want = np.stack([download(hipmem, o[k], total) for k in range(3)], axis=1)
    want_i, want_cnt = download(hipmem, o[3], total), download(hipmem, o_cnt, total, np.int32)
    out, cnt = sentinel_cloud(total + 2, cols), np.full(total + 2, -9, np.int32)
    rc, m = map_export_host(pkg, ndt, cols, icol, out, cnt, total)
    assert rc == 0 and m == total
    check_written(out, m, cols, icol, want, want_i)
    assert np.array_equal(cnt[:m], want_cnt) and np.all(cnt[m:] == -9)
    assert total > 1 or n == 1
    if total > 1:   # one voxel too few: the voxels that fit are written, then the call fails with the total
        out, cnt = sentinel_cloud(total + 2, cols), np.full(total + 2, -9, np.int32)
        rc, m = map_export_host(pkg, ndt, cols, icol, out, cnt, total - 1)
        assert rc == INVALID_ARG and m == total and ("%d voxels" % total) in last_error(pkg, ndt)
        check_written(out, total - 1, cols, icol, want, want_i)
        assert np.array_equal(cnt[:total - 1], want_cnt[:total - 1]) and np.all(cnt[total - 1:] == -9)
    ndt.mapClear()


def random_model(n_cols, n_rows, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(3, n_cols, n_rows))
    d /= np.linalg.norm(d, axis=0)
    return [d[k].astype(np.float32) for k in range(3)] + [rng.uniform(-0.05, 0.05, n_cols).astype(np.float32) for _ in range(3)]


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("n_cols,n_rows", [(1, 1), (13, 5), (60, 50)])
@pytest.mark.parametrize("cols,icol", LAYOUTS)
def test_unproject(pkg, ndt, hipmem, cols, icol, n_cols, n_rows, compact):
    n = n_cols * n_rows
    rng = np.random.default_rng(71 + n)
    ndt.setScanModel(*random_model(n_cols, n_rows, 70 + n))
    try:
        r = rng.integers(500, 100000, n).astype(np.uint32)
        if n > 1:
            r[::6] = 0                                      # (no return: NaN in the organised form, dropped by a filter)
        refl = rng.integers(0, 256, n).astype(np.uint8)
        col_t = rng.uniform(0.0, 1.0, n_cols).astype(np.float32)
        filt = pkg.ScanFilter() if compact else None
        d_r, d_refl, d_ct = hipmem.upload(r), hipmem.upload(refl), hipmem.upload(col_t)
        o, d_idx = device_out(hipmem, n, 5), hipmem.upload(np.zeros(n, np.int32))
        m_dev = ndt.unprojectDevice(d_r, d_refl if icol is not None else None, d_ct, o[0], o[1], o[2], n, knot_t=KNOT_T,
                                    knot_poses=knot_poses(), filter=filt, o_intensity=o[3] if icol is not None else None, o_t=o[4],
                                    d_index=d_idx)
        assert m_dev == (np.count_nonzero(r) if compact else n)
        want = np.stack([download(hipmem, o[k], m_dev) for k in range(3)], axis=1)
        want_i, want_t, want_idx = download(hipmem, o[3], m_dev), download(hipmem, o[4], m_dev), download(hipmem, d_idx, m_dev, np.int32)
        out = sentinel_cloud(n + 2, cols)
        tt, idx = np.full(n + 2, SENTINEL, np.uint32).view(np.float32), np.full(n + 2, -9, np.int32)
        kt, poses, nk, ref = ndt._trajectory_or_none(KNOT_T, knot_poses(), None)
        m = C.c_size_t(0)
        rc = pkg.lib().ndt_unproject(ndt._h, r.ctypes.data, refl.ctypes.data if icol is not None else None, col_t.ctypes.data, None, kt,
                                     poses, nk, ref, ndt._filter_ref(filt), out.ctypes.data, 4 * cols, -1 if icol is None else 4 * icol,
                                     tt.ctypes.data, idx.ctypes.data, n, C.byref(m))
        assert rc == 0 and m.value == m_dev
        check_written(out, m_dev, cols, icol, want, want_i)
        assert np.array_equal(bits(tt[:m_dev]), bits(want_t)) and np.all(bits(tt[m_dev:]) == SENTINEL)
        assert np.array_equal(idx[:m_dev], want_idx) and np.all(idx[m_dev:] == -9)
    finally:
        ndt.clearScanModel()


@pytest.mark.parametrize("n", SIZES[1:])
def test_filter_source_and_transform_source_ct(pkg, ndt, hipmem, n):
    """tight clouds (a stride of 12 bytes, no intensity): the rows behind the result keep the sentinel"""
    world, _, _ = make_cloud(3000, 3, None, 5)
    _, src, _ = make_cloud(n, 3, None, 83 + n)
    ndt.setInputTarget(world)
    ndt.setInputSource(src)
    T = np.ascontiguousarray(np.eye(4, dtype=np.float32).T).ravel()
    o, d_idx = device_out(hipmem, n, 3), hipmem.upload(np.zeros(n, np.int32))
    for thr in (0.0, 0.3):                                 # (a score is never negative: 0.0 selects every point)
        m_dev = ndt.filterSourceDevice(np.eye(4), thr, False, o[0], o[1], o[2], d_idx, n)
        assert m_dev == n or thr > 0.0
        want = np.stack([download(hipmem, o[k], m_dev) for k in range(3)], axis=1)
        want_idx = download(hipmem, d_idx, m_dev, np.int32)
        out, idx = sentinel_cloud(n + 2, 3), np.full(n + 2, -9, np.int32)
        m = C.c_size_t(0)
        rc = pkg.lib().ndt_filter_source(ndt._h, pkg._fp(T), thr, 0, out.ctypes.data, idx.ctypes.data, n, C.byref(m))
        assert rc == 0 and m.value == m_dev
        check_written(out, m_dev, 3, None, want, None)
        assert np.array_equal(idx[:m_dev], want_idx) and np.all(idx[m_dev:] == -9)
    # the continuous-time transform of the source
    pkg.setSourceTimes(ndt, np.linspace(0.0, 1.0, n).astype(np.float32))
    begin, end = np.zeros(6), np.array([0.5, -0.25, 0.1, 0.01, -0.02, 0.2])
    pkg.transformSourceCTDevice(ndt, begin, end, o[0], o[1], o[2], n)
    want = np.stack([download(hipmem, o[k], n) for k in range(3)], axis=1)
    out = sentinel_cloud(n + 2, 3)
    b, e = np.ascontiguousarray(begin, np.float64), np.ascontiguousarray(end, np.float64)
    rc = pkg.lib().ndt_transform_source_ct(ndt._h, pkg._dp(b), pkg._dp(e), 0, out.ctypes.data, n)
    assert rc == 0
    check_written(out, n, 3, None, want, None)
    assert not np.array_equal(want, src)
