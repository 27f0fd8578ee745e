"""Deskew on the device (ndt_deskew_device / ndt_deskew / ndt_keyframe_put_deskewed) against the NumPy f64 reference of
tests/test_deskew_cpu.py -- the geodesic R_k Exp(u Log(R_k^T R_{k+1})), not the product's slerp.

Tolerance of every point comparison: |out - ref64| <= 0.5 ulp_f32(|ref64|) + 1e-9 m per coordinate -- the one f32
rounding the product is allowed, plus 1e-9, three orders above f64 round-off at 300 m (about 3e-12) and four below the
f32 spacing there (1.5e-5).  No case is left out of a comparison.

Compaction boundaries: the kernels work in blocks of 256 points and ONE block of 1024 threads scans the block counts, 1024
per pass: 262 144 = 1024 x 256 points is where the scan starts its second pass (tested with its neighbours)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_deskew_cpu import (SEGMENT_ROTATIONS, assert_points_within_tolerance, deskew_numpy, make_trajectory, poses_numpy,
                             ref_choices)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHOR_SIZES = [1, 63, 64, 65, 255, 256, 257, 1025]
COMPACT_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 262143, 262144, 262145, 300001]


@pytest.fixture(scope="module")
def ndt(pkg):
    e = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=50)
    yield e
    e.close()


def download(hipmem, ptr, n, dtype=np.float32):
    out = np.zeros(n, dtype)
    if n:
        assert hipmem.rt.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return out


def random_scan(n, seed, radius=250.0):
    """n points of |p| up to `radius` m, an intensity in [0, 255) and a time in [-0.2, 1.2)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
    pts = (d * rng.uniform(0.0, radius, (n, 1))).astype(np.float32)
    return pts, rng.uniform(0.0, 255.0, n).astype(np.float32), rng.uniform(-0.2, 1.2, n).astype(np.float32)


def f32_knots(kt):
    """knot times a float can hit exactly (still strictly increasing: the steps are around 0.1)"""
    out = np.asarray(kt, np.float32).astype(np.float64)
    assert np.all(np.diff(out) > 0)
    return out


def device_deskew(ndt, hipmem, pts, t, kt, kp, ref=None, filt=None, inten=None, cap=None, in_place=False, fill=None, alloc=None):
    """ndt_deskew_device on uploaded SoA arrays -> (xyz [m, 3], intensity [m] or None, index [m], m); the whole output
    arrays as downloaded are kept in device_deskew.last_raw.  alloc: elements the output arrays hold (default: cap)."""
    n = len(pts)
    cap = n if cap is None else cap
    alloc = cap if alloc is None else alloc
    din = [hipmem.upload(np.ascontiguousarray(pts[:, a])) for a in range(3)]
    dt = hipmem.upload(t)
    di = None if inten is None else hipmem.upload(inten)
    init = np.full(max(alloc, 1), np.nan if fill is None else fill, np.float32)
    dout = din if in_place else [hipmem.upload(init) for _ in range(3)]
    doi = None if inten is None else hipmem.upload(init)
    didx = hipmem.upload(np.full(max(alloc, 1), -7, np.int32))
    try:
        m = ndt.deskewDevice(din[0], din[1], din[2], dt, n, kt, kp, dout[0], dout[1], dout[2], cap, ref_pose=ref, filter=filt,
                             d_intensity=di, o_intensity=doi, d_index=didx)
    finally:
        size = n if in_place else alloc
        raw = dict(xyz=np.stack([download(hipmem, p, size) for p in dout], 1),
                   intensity=None if inten is None else download(hipmem, doi, alloc),
                   index=download(hipmem, didx, alloc, np.int32))
        device_deskew.last_raw = raw
    return raw["xyz"][:m], None if inten is None else raw["intensity"][:m], raw["index"][:m], m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def read_source(pkg, ndt):
    """the current source as the engine holds it (ndt_transform_source with the identity)"""
    n = ndt.sourceSize()
    out = np.zeros((n, 3), np.float32)
    eye = np.eye(4, dtype=np.float32).ravel()
    if n:
        assert pkg.lib().ndt_transform_source(ndt._h, eye.ctypes.data_as(C.POINTER(C.c_float)),
                                              out.ctypes.data_as(C.POINTER(C.c_float)), n) == 0
    return out


# ---- 1. exactness anchors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ANCHOR_SIZES)
def test_no_motion_is_exact(pkg, ndt, hipmem, n):
    """every knot equal to the reference: output bit-equal to input -- aligned, aligned in place, compacting with a zeroed
    filter and no non-finite point; -0.0 and denormals included"""
    pts, inten, t = random_scan(n, 100 + n)
    pts[0] = [-0.0, 1e-42, -1e-40][:3]
    for n_knots in (1, 2, 64):
        _, one = make_trajectory(1, 7 + n_knots)
        kp = np.repeat(one, n_knots, axis=0)
        kt = np.linspace(0.0, 1.0, n_knots) if n_knots > 1 else np.array([0.5])
        for ref in (None, one[0]):
            for kw in (dict(), dict(in_place=True), dict(filt=pkg.ScanFilter())):
                xyz, oi, idx, m = device_deskew(ndt, hipmem, pts, t, kt, kp, ref=ref, inten=inten, **kw)
                assert m == n
                assert np.array_equal(bits(xyz), bits(pts)), (n_knots, kw.keys())
                assert np.array_equal(bits(oi), bits(inten)) and np.array_equal(idx, np.arange(n))
                hipmem.free_all()
        out, hidx = ndt.deskew(np.column_stack([pts, inten]), t, kt, kp, intensity_column=3, with_index=True)
        assert np.array_equal(bits(out), bits(np.column_stack([pts, inten]))) and np.array_equal(hidx, np.arange(n))


# ---- 2. model parity --------------------------------------------------------------------------------------------------
def parity_scan(kt, seed, n=4099):
    """points of |p| up to 250 m; times on every knot, outside both ends, and between the knots"""
    pts, inten, t = random_scan(n, seed)
    span = kt[-1] - kt[0]
    t = (kt[0] + (t.astype(np.float64) * span)).astype(np.float32)      # [-0.2, 1.2) of the knots' range
    t[:len(kt)] = kt.astype(np.float32)
    assert np.array_equal(t[:len(kt)].astype(np.float64), kt)           # exactly ON the knots
    assert (t < kt[0]).any() and (t > kt[-1]).any()
    return pts, inten, t


PARITY = [(2, r) for r in range(len(SEGMENT_ROTATIONS))] + [(3, 0), (3, 2), (3, 3), (22, 0), (64, 0)]


@pytest.mark.parametrize("n_knots,first", PARITY)
def test_matches_the_geodesic_reference(pkg, S, ndt, hipmem, n_knots, first):
    rots = SEGMENT_ROTATIONS[first:] + SEGMENT_ROTATIONS[:first]
    kt, kp = make_trajectory(n_knots, 50 + 7 * n_knots + first, rots)
    kt = f32_knots(kt)
    pts, inten, t = parity_scan(kt, 900 + n_knots + first)
    for name, ref in ref_choices(kp, n_knots + first):
        want = deskew_numpy(S, pts, t, kt, kp, ref)
        xyz, _, idx, m = device_deskew(ndt, hipmem, pts, t, kt, kp, ref=ref)
        assert m == len(pts) and np.array_equal(idx, np.arange(m))
        assert_points_within_tolerance(xyz, want, "aligned, %d knots, first rotation %g, ref %s" % (n_knots, rots[0], name))
        xyz, _, idx, m = device_deskew(ndt, hipmem, pts, t, kt, kp, ref=ref, filt=pkg.ScanFilter())
        assert m == len(pts)
        assert_points_within_tolerance(xyz, want, "compacting, %d knots, ref %s" % (n_knots, name))
        hipmem.free_all()
    host = ndt.deskew(pts, t, kt, kp)
    assert_points_within_tolerance(host, deskew_numpy(S, pts, t, kt, kp), "host form, %d knots" % n_knots)


def test_non_finite_points_give_nan_in_the_aligned_mode(pkg, S, ndt, hipmem):
    kt, kp = make_trajectory(3, 21)
    pts, inten, t = random_scan(300, 5)
    t = (t * kt[-1]).astype(np.float32)
    pts[3, 0], pts[64, 1], pts[65, 2], pts[299, 0] = np.nan, np.inf, -np.inf, np.nan
    t[10], t[255], t[256] = np.nan, np.inf, -np.inf
    want = deskew_numpy(S, pts, t, kt, kp)
    assert np.isnan(want).all(1).sum() == 7
    xyz, oi, _, m = device_deskew(ndt, hipmem, pts, t, kt, kp, inten=inten, fill=0.0)
    assert m == 300 and np.array_equal(bits(oi), bits(inten))
    assert_points_within_tolerance(xyz, want, "non-finite points")


# ---- 3. compaction boundaries -----------------------------------------------------------------------------------------
def keep_numpy(f, pts, t, inten):
    """the predicate of include/ndt_hip.h on the raw f32 values"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(t)
        if f.use_box:
            lo, hi = np.array(f.box_min[:], np.float32), np.array(f.box_max[:], np.float32)
            keep &= ~((lo[0] <= x) & (x <= hi[0]) & (lo[1] <= y) & (y <= hi[1]) & (lo[2] <= z) & (z <= hi[2]))
        if f.use_z_or_intensity:
            band = (np.float32(f.z_min) <= z) & (z <= np.float32(f.z_max))
            bright = np.zeros(len(pts), bool) if inten is None else inten >= np.float32(f.intensity_keep_min)
            keep &= band | bright
    return keep


@pytest.mark.parametrize("n", COMPACT_SIZES)
def test_compaction_matches_the_boolean_mask(pkg, S, ndt, hipmem, n):
    kt, kp = make_trajectory(3, 33)
    pts, inten, t = random_scan(n, 300 + n % 1000, radius=60.0)
    t = (t * kt[-1]).astype(np.float32)
    f = pkg.ScanFilter.from_vehicle_box(None, None, z_band=(0.0, 1.0))       # keep = (0 <= z <= 1)
    rng = np.random.default_rng(n)
    patterns = dict(none=np.zeros(n, bool), all=np.ones(n, bool), alternate=np.arange(n) % 2 == 0,
                    last=np.arange(n) == n - 1, random30=rng.uniform(size=n) < 0.3)
    orig = pts.copy()
    moved, _, _, _ = device_deskew(ndt, hipmem, pts, t, kt, kp) if n else (np.zeros((0, 3), np.float32), None, None, 0)
    hipmem.free_all()
    for name, want in patterns.items():
        pts[:, 2] = np.where(want, np.float32(0.5), np.float32(5.0))
        assert np.array_equal(keep_numpy(f, pts, t, None), want)
        aligned, _, _, _ = device_deskew(ndt, hipmem, pts, t, kt, kp) if n else (moved, None, None, 0)
        xyz, oi, idx, m = device_deskew(ndt, hipmem, pts, t, kt, kp, filt=f, inten=inten, fill=-1.0)
        sel = np.flatnonzero(want)
        assert m == len(sel), (name, m, len(sel))
        assert np.array_equal(idx, sel), name
        assert np.array_equal(bits(xyz), bits(aligned[sel])), name          # the same arithmetic as the aligned launch
        assert np.array_equal(bits(oi), bits(inten[sel])), name
        raw = device_deskew.last_raw                                        # nothing behind the kept points
        assert np.all(raw["xyz"][m:] == -1.0) and np.all(raw["index"][m:] == -7), name
        hipmem.free_all()
    if n:
        assert_points_within_tolerance(moved, deskew_numpy(S, orig, t, kt, kp), "n = %d" % n)


def test_predicate_edges(pkg, ndt, hipmem):
    """points exactly on every face of the box and on z_min, z_max and intensity_keep_min (all inclusive); NaN / Inf in x,
    in t and in intensity; no intensity array with the z band on"""
    f = pkg.ScanFilter.from_vehicle_box([0.5, 0.0, 0.25], [3.0, 2.0, 1.5], z_band=(-2.0, 1.5), intensity_keep_min=100.0)
    lo, hi = np.array(f.box_min[:], np.float32), np.array(f.box_max[:], np.float32)
    assert list(lo) == [-1.0, -1.0, -0.5] and list(hi) == [2.0, 1.0, 1.0]
    up, down = (lambda v: np.nextafter(np.float32(v), np.float32(np.inf))), (lambda v: np.nextafter(np.float32(v), np.float32(-np.inf)))
    rows, expect = [], []

    def add(x, y, z, inten, t, keep):
        rows.append((x, y, z, inten, t))
        expect.append(keep)

    mid = 0.5 * (lo + hi)
    for a in range(3):
        for face, outside in ((lo[a], down(lo[a])), (hi[a], up(hi[a]))):
            p = mid.copy()
            p[a] = face
            add(*p, 0.0, 0.5, False)                                # ON a face: inside the box, rejected
            p[a] = outside
            add(*p, 0.0, 0.5, True)                                 # one ulp outside: not in the box, z inside the band
    add(5.0, 5.0, -2.0, 0.0, 0.5, True)                             # z == z_min
    add(5.0, 5.0, 1.5, 0.0, 0.5, True)                              # z == z_max
    add(5.0, 5.0, down(-2.0), 0.0, 0.5, False)
    add(5.0, 5.0, up(1.5), 0.0, 0.5, False)
    add(5.0, 5.0, 9.0, 100.0, 0.5, True)                            # intensity == intensity_keep_min
    add(5.0, 5.0, 9.0, down(100.0), 0.5, False)
    add(5.0, 5.0, 9.0, np.inf, 0.5, True)
    add(5.0, 5.0, 9.0, np.nan, 0.5, False)
    add(5.0, 5.0, 0.0, np.nan, 0.5, True)                           # (the band alone keeps it)
    add(mid[0], mid[1], mid[2], 255.0, 0.5, False)                  # bright, but inside the box
    for bad in (np.nan, np.inf, -np.inf):
        add(bad, 5.0, 0.0, 255.0, 0.5, False)
        add(5.0, bad, 0.0, 255.0, 0.5, False)
        add(5.0, 5.0, bad, 255.0, 0.5, False)
        add(5.0, 5.0, 0.0, 255.0, bad, False)
    a = np.array(rows, np.float32)
    a = np.tile(a, (5, 1))                                          # several waves, edges on different lanes
    want = np.tile(np.array(expect), 5)
    pts, inten, t = np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(a[:, 3]), np.ascontiguousarray(a[:, 4])
    assert np.array_equal(keep_numpy(f, pts, t, inten), want)       # the NumPy predicate against the hand-made list
    kt, kp = make_trajectory(2, 3)
    _, oi, idx, m = device_deskew(ndt, hipmem, pts, t, kt, kp, filt=f, inten=inten)
    assert m == want.sum() and np.array_equal(idx, np.flatnonzero(want))
    assert np.array_equal(bits(oi), bits(inten[want]))
    # no intensity array: the second alternative is false for every point
    no_i = keep_numpy(f, pts, t, None)
    assert no_i.sum() < want.sum()
    _, _, idx, m = device_deskew(ndt, hipmem, pts, t, kt, kp, filt=f)
    assert m == no_i.sum() and np.array_equal(idx, np.flatnonzero(no_i))
    # a zeroed filter: the finite points
    fin = keep_numpy(pkg.ScanFilter(), pts, t, inten)
    _, _, idx, m = device_deskew(ndt, hipmem, pts, t, kt, kp, filt=pkg.ScanFilter(), inten=inten)
    assert m == fin.sum() == len(pts) - 60 and np.array_equal(idx, np.flatnonzero(fin))
    # the host form, with its index
    out, hidx = ndt.deskew(a[:, :4], t, kt, kp, filter=f, intensity_column=3, with_index=True)
    assert np.array_equal(hidx, np.flatnonzero(want)) and np.array_equal(bits(out[:, 3]), bits(inten[want]))


def test_capacity_and_argument_refusals(pkg, ndt, hipmem):
    kt, kp = make_trajectory(3, 8)
    pts, inten, t = random_scan(1000, 77, radius=50.0)
    t = (t * kt[-1]).astype(np.float32)
    f = pkg.ScanFilter.from_vehicle_box(None, None, z_band=(-10.0, 10.0))
    want = keep_numpy(f, pts, t, None)
    m = int(want.sum())
    assert 100 < m < 1000
    full, full_i, full_idx, got = device_deskew(ndt, hipmem, pts, t, kt, kp, filt=f, inten=inten)
    assert got == m
    # cap < n_out: refused with the count; the outputs HOLD n elements, so a write beyond cap would be seen
    cap = m - 3
    with pytest.raises(pkg.NdtError) as e:
        device_deskew(ndt, hipmem, pts, t, kt, kp, filt=f, inten=inten, cap=cap, alloc=len(pts), fill=-1.0)
    assert e.value.code == -1 and str(m) in str(e.value) and ndt.last_deskew_count == m
    raw = device_deskew.last_raw
    assert len(raw["xyz"]) == len(raw["intensity"]) == len(raw["index"]) == len(pts)
    assert np.all(raw["xyz"][cap:] == -1.0) and np.all(raw["intensity"][cap:] == -1.0) and np.all(raw["index"][cap:] == -7)
    assert np.array_equal(bits(raw["xyz"][:cap]), bits(full[:cap]))     # what was written is the first cap of the selection
    assert np.array_equal(bits(raw["intensity"][:cap]), bits(full_i[:cap])) and np.array_equal(raw["index"][:cap], full_idx[:cap])
    # ... and through the host form: rows at and beyond cap (here: every row) untouched, *n_out the number selected
    cloud = np.column_stack([pts, inten])
    out, hidx, n_out = np.full((len(pts), 4), -1.0, np.float32), np.full(len(pts), -7, np.int32), C.c_size_t(0)
    kt64, poses = np.ascontiguousarray(kt, np.float64), np.ascontiguousarray(np.transpose(kp, (0, 2, 1))).ravel()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    rc = pkg.lib().ndt_deskew(ndt._h, cloud.ctypes.data, len(cloud), 16, 12, t.ctypes.data, dp(kt64), dp(poses), 3, None, C.byref(f),
                              out.ctypes.data, hidx.ctypes.data, cap, C.byref(n_out))
    assert rc == -1 and n_out.value == m and str(m) in pkg.lib().ndt_last_error(ndt._h).decode()
    assert np.all(out[cap:] == -1.0) and np.all(hidx[cap:] == -7) and np.all(out == -1.0)
    rc = pkg.lib().ndt_deskew(ndt._h, cloud.ctypes.data, len(cloud), 16, 12, t.ctypes.data, dp(kt64), dp(poses), 3, None, C.byref(f),
                              out.ctypes.data, hidx.ctypes.data, m, C.byref(n_out))     # cap == n_out: exactly enough
    assert rc == 0 and n_out.value == m and np.all(out[m:] == -1.0) and np.all(hidx[m:] == -7)
    assert np.array_equal(bits(out[:m, :3]), bits(full)) and np.array_equal(hidx[:m], full_idx)
    # aligned: cap >= n, refused before anything is written, *n_out = n in both forms
    with pytest.raises(pkg.NdtError) as e:
        device_deskew(ndt, hipmem, pts, t, kt, kp, cap=999, alloc=1000, fill=-1.0)
    assert "1000" in str(e.value) and np.all(device_deskew.last_raw["xyz"] == -1.0) and ndt.last_deskew_count == 1000
    out[:] = -1.0
    rc = pkg.lib().ndt_deskew(ndt._h, cloud.ctypes.data, len(cloud), 16, 12, t.ctypes.data, dp(kt64), dp(poses), 3, None, None,
                              out.ctypes.data, None, 999, C.byref(n_out))
    assert rc == -1 and n_out.value == 1000 and np.all(out == -1.0)
    with pytest.raises(pkg.NdtError):
        ndt.deskew(pts, t, kt[::-1].copy(), kp)                      # times not increasing
    archived = ndt.keyframeCount()
    with pytest.raises(pkg.NdtError):
        ndt.putKeyframeDeskewed(991, pts, t, [0.0, np.nan, 1.0], kp)
    assert ndt.keyframeCount() == archived
    # a compacted output must not overlap an input; refused as a whole
    d = [hipmem.upload(np.ascontiguousarray(pts[:, a])) for a in range(3)]
    dt = hipmem.upload(t)
    o = [hipmem.upload(np.full(1000, -1.0, np.float32)) for _ in range(2)]
    with pytest.raises(pkg.NdtError) as e:
        ndt.deskewDevice(d[0], d[1], d[2], dt, 1000, kt, kp, o[0], o[1], d[2] + 4 * 999, 1000, filter=f)
    assert "overlap" in str(e.value)
    assert np.all(download(hipmem, o[0], 1000) == -1.0) and np.array_equal(download(hipmem, d[2], 1000), pts[:, 2])
    # aligned: an output may BE an input array (tested in place above), but must not overlap one otherwise
    for bad in (d[0] + 4, d[1] - 4):
        with pytest.raises(pkg.NdtError) as e:
            ndt.deskewDevice(d[0], d[1], d[2], dt, 1000, kt, kp, bad, o[0], o[1], 1000)
        assert "overlap" in str(e.value)
    assert np.array_equal(download(hipmem, d[0], 1000), pts[:, 0]) and np.all(download(hipmem, o[0], 1000) == -1.0)
    assert ndt.deskewDevice(d[0], d[1], d[2], dt, 0, kt, kp, o[0], o[1], o[0], 0, filter=f) == 0   # n = 0: a no-op


# ---- 4. the three forms agree -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [12, 16, 32])
def test_three_forms_agree(pkg, S, ndt, hipmem, stride):
    kt, kp = make_trajectory(22, 61, [np.deg2rad(0.3), 1e-5, np.deg2rad(1.0)], trans=0.1)
    pts, inten, t = random_scan(5003, 62, radius=120.0)
    t = (t * kt[-1]).astype(np.float32)
    pts[11, 1], t[4000] = np.nan, np.inf
    cols = stride // 4
    cloud = np.zeros((len(pts), cols), np.float32)
    cloud[:, :3] = pts
    icol = None if cols == 3 else (3 if cols == 4 else 4)
    if icol is not None:
        cloud[:, icol] = inten
    f = pkg.ScanFilter.from_vehicle_box([0.0, 0.0, 0.0], [40.0, 40.0, 40.0], z_band=(-30.0, 30.0), intensity_keep_min=200.0)
    for filt in (None, pkg.ScanFilter(), f):
        host, hidx = ndt.deskew(cloud, t, kt, kp, filter=filt, intensity_column=icol, with_index=True)
        xyz, oi, idx, m = device_deskew(ndt, hipmem, pts, t, kt, kp, filt=filt, inten=None if icol is None else inten)
        assert len(host) == m and (m == len(pts) if filt is None else m < len(pts))
        assert np.array_equal(bits(host[:, :3]), bits(xyz)) and np.array_equal(hidx, idx)
        if icol is not None:
            assert np.array_equal(bits(host[:, icol]), bits(oi))
        if filt is not None:
            assert np.array_equal(idx, np.flatnonzero(keep_numpy(filt, pts, t, None if icol is None else inten)))
        assert ndt.putKeyframeDeskewed(5, cloud, t, kt, kp, filter=filt, intensity_column=icol) == m
        ndt.setInputSourceFromKeyframe(5)
        back = read_source(pkg, ndt)
        assert back.shape == xyz.shape and np.array_equal(back, xyz, equal_nan=True)
        # replacing the keyframe that is the viewed source unsets the source, as ndt_keyframe_put does
        assert ndt.putKeyframeDeskewed(5, cloud, t, kt, kp, filter=filt, intensity_column=icol) == m
        assert ndt.sourceSize() == 0
        hipmem.free_all()
    ndt.eraseKeyframe(5)


def test_deskew_leaves_the_engine_state_alone(pkg, S, ndt, hipmem):
    cfg = S.config_c1(max_points=4000)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    T1 = ndt.align(cfg["guess"])
    hist1, leaves1, src1 = ndt.getIterationHistory(), ndt.getLeaves(), read_source(pkg, ndt)
    kt, kp = make_trajectory(5, 13)
    pts, inten, t = random_scan(3000, 14)
    ndt.deskew(pts, t, kt, kp)
    ndt.deskew(np.column_stack([pts, inten]), t, kt, kp, filter=pkg.ScanFilter(), intensity_column=3)
    device_deskew(ndt, hipmem, pts, t, kt, kp, filt=pkg.ScanFilter())
    ndt.putKeyframeDeskewed(77, pts, t, kt, kp)
    hist2, leaves2 = ndt.getIterationHistory(), ndt.getLeaves()
    for a, b in zip(hist1, hist2):
        assert a.tobytes() == b.tobytes()
    assert sorted(leaves1) == sorted(leaves2)
    for k in leaves1:
        assert np.asarray(leaves1[k]).tobytes() == np.asarray(leaves2[k]).tobytes(), k
    assert read_source(pkg, ndt).tobytes() == src1.tobytes()
    T2 = ndt.align(cfg["guess"])
    assert T1.tobytes() == T2.tobytes()
    for a, b in zip(hist1, ndt.getIterationHistory()):
        assert a.tobytes() == b.tobytes()
    ndt.eraseKeyframe(77)


# ---- 5. it fixes what it is for ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moving_scan(S):
    """A scan taken while the sensor moves from Tbeg to Tend: the ideal scan P at Tend, and the raw scan as the sensor
    delivers it -- every point in the sensor frame of ITS instant alpha = azimuth / 2 pi."""
    sim = S.OusterSim(S.Scene(seed=42), beams=32, cols=256)
    Ta = S.pose_matrix(0.0, 0.0, 2.0, 0.0, 0.0, 0.0)
    Tend = Ta @ S.pose_matrix(0.5, 0.1, 0.0, 0.0, 0.0, np.deg2rad(2.0))
    Tbeg = Tend @ np.linalg.inv(S.pose_matrix(1.0, 0.05, 0.0, 0.0, 0.01, np.deg2rad(3.0)))
    P = sim.scan(Tend, seed=44)
    alpha = (np.mod(np.arctan2(P[:, 1].astype(np.float64), P[:, 0].astype(np.float64)), 2.0 * np.pi) / (2.0 * np.pi)).astype(np.float32)
    kt, kp = np.array([0.0, 1.0]), np.stack([Tbeg, Tend])
    # W = Tend P, raw = T(alpha)^-1 W = D(alpha)^-1 P with D(alpha) = Tend^-1 T(alpha)
    R, d = poses_numpy(S, kt, kp, alpha.astype(np.float64), Tend)
    raw = np.einsum("mji,mj->mi", R, P.astype(np.float64) - d).astype(np.float32)
    s = np.linspace(0.0, 1.0, 22)
    R22, d22 = poses_numpy(S, kt, kp, s, Tend)
    kp22 = np.stack([Tend @ np.block([[R22[k], d22[k][:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]) for k in range(22)])
    kp22[-1] = Tend
    return dict(target=sim.scan(Ta, seed=43), P=P, raw=raw, alpha=alpha, gt=np.linalg.inv(Ta) @ Tend, kt=kt, kp=kp, kt22=s, kp22=kp22)


@pytest.mark.parametrize("knots", [2, 22])
def test_deskewed_scan_aligns_like_the_ideal_scan(pkg, S, moving_scan, knots):
    """Oracle figures for this set-up (CPU, 1.0 m voxels): ideal 0.071 m / 1.2 mrad to ground truth, raw 0.72 m / 37 mrad,
    deskewed within 1.1 mm / 0.07 mrad of the ideal result.  Required here: deskewed within 5 mm / 0.5 mrad of the ideal
    result (Newton stops at trans_epsilon = 1e-4: the two runs may differ by an iteration or two), and the raw scan's
    error to ground truth at least 5 x the deskewed scan's."""
    c = moving_scan
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=50)
    try:
        ndt.setInputTarget(c["target"])
        kt, kp = (c["kt"], c["kp"]) if knots == 2 else (c["kt22"], c["kp22"])
        desk = ndt.deskew(c["raw"], c["alpha"], kt, kp)
        T = {}
        for name, src in (("ideal", c["P"]), ("raw", c["raw"]), ("deskewed", desk)):
            ndt.setInputSource(src)
            T[name] = ndt.align(np.eye(4))
    finally:
        ndt.close()
    err = {k: S.pose_error(T[k], c["gt"]) for k in T}
    to_ideal = S.pose_error(T["deskewed"], T["ideal"])
    print("%d knots | to ground truth: ideal %.4f m %.5f rad, raw %.4f m %.5f rad, deskewed %.4f m %.5f rad | deskewed to ideal "
          "%.5f m %.6f rad | deskewed scan to ideal scan, max |dp| %.2e m"
          % (knots, *err["ideal"], *err["raw"], *err["deskewed"], *to_ideal, float(np.abs(desk - c["P"]).max())))
    assert to_ideal[0] <= 5e-3 and to_ideal[1] <= 0.5e-3
    assert err["raw"][0] >= 5.0 * err["deskewed"][0] and err["raw"][1] >= 5.0 * err["deskewed"][1]


# ---- 6. the C++ face --------------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, tmp_path):
    """tests/cpp/test_deskew.cpp against the API mocks, built with the g++ line tests/cpp/Makefile uses for test_driver_shape."""
    d = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "test_deskew")
    lib = os.path.join(ROOT, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(ROOT, "include", "compat"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(d, "test_deskew.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "deskew: PASS" in p.stdout
