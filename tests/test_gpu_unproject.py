"""Unprojection of a range image on the device (ndt_unproject_device / ndt_unproject / ndt_keyframe_put_from_ranges) against
two references, no case left out of any comparison:
  * the exact fused multiply-add of the f32 operands, rounded once to f32, computed on the host (fma_f32 below: the
    product of two floats is exact in float64, TwoSum gives the sum's error, and a float64 sum that lands on the midpoint
    of two floats is pushed off it by that error -- checked against fractions.Fraction at every small shape);
  * ndt_deskew_device on the organised output: the fused calls must return its bits.
Compaction boundaries: blocks of 256 pixels, ONE block of 1024 threads scans the block counts, 1024 per pass: 262 144 =
1024 x 256 pixels is where the scan starts its second pass (tested with its neighbours)."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_deskew_cpu import make_trajectory, ref_choices
from test_gpu_deskew import bits, device_deskew, download, f32_knots, keep_numpy, read_source
from test_unproject_cpu import SURFACE_BOUND, moving_scene, surface_distance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORGANISED_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 85), (2, 128), (257, 1), (5, 205)]
COMPACT_SHAPES = [(5, 51), (2, 128), (257, 1), (511, 513), (2048, 128), (2049, 128), (300001, 1)]
SPECIAL_RANGES = [0, 1, 2 ** 19 - 1, 2 ** 20 - 1]
STATE = {"organised_failed": False}


@pytest.fixture(scope="module")
def ndt(pkg):
    e = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=50)
    yield e
    e.close()


# --------------------------------------------------------------------------- references
def fma_f32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, exactly: one rounding of the exact a * b + c"""
    a64, b64, c64 = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a64 * b64                                         # exact: 24 + 24 bits
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)                       # TwoSum: p + c64 = s + e exactly
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    toward = np.where(r64 > s, -np.inf, np.inf).astype(np.float32)
    other = np.nextafter(r, toward)
    tie = (r64 != s) & (np.abs(r64 - s) == np.abs(other.astype(np.float64) - s))
    # on a tie float64 -> float32 went to even; the exact value lies on the side of e
    wrong = tie & (((r64 > s) & (e < 0.0)) | ((r64 < s) & (e > 0.0)))
    return np.where(wrong, other, r).astype(np.float32)


def fma_fraction(a, b, c):
    """the same through fractions.Fraction, one value at a time (the check of fma_f32)"""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    r = np.float32(float(exact))                          # (Fraction -> float64 is correctly rounded; the float32 is a candidate)
    best = min((np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf))),
               key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def random_model(n_cols, n_rows, seed):
    """unit directions anywhere on the sphere and offsets of a few centimetres, every entry non-zero"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_cols, n_rows, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    o = rng.uniform(-0.05, 0.05, (n_cols, 3))
    m = [np.ascontiguousarray(d[:, :, a], np.float32) for a in range(3)] + [np.ascontiguousarray(o[:, a], np.float32) for a in range(3)]
    assert all(np.all(a != 0.0) for a in m)
    return tuple(m)


def random_image(n_cols, n_rows, seed, zero_share=0.15, nan_cols=True, span=1.0):
    """ranges over the whole 20 bits with the special values and a share of zeros, reflectivities over the whole byte,
    column times in [-0.2, 1.2) x span (outside the knots on either side) of which some are NaN or Inf"""
    rng = np.random.default_rng(seed)
    n = n_cols * n_rows
    r = rng.integers(1, 2 ** 20, n).astype(np.uint32)
    r[rng.uniform(size=n) < zero_share] = 0
    where = rng.permutation(n)[:len(SPECIAL_RANGES)]
    r[where] = SPECIAL_RANGES[:len(where)]
    refl = rng.integers(0, 256, n).astype(np.uint8)
    refl[rng.permutation(n)[:2]] = [0, 255][:min(n, 2)]
    t = (rng.uniform(-0.2, 1.2, n_cols) * span).astype(np.float32)
    if nan_cols and n_cols >= 3:
        bad = rng.permutation(n_cols)[:max(1, n_cols // 8)]
        t[bad] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(len(bad)) % 3]
    return r.reshape(n_cols, n_rows), refl.reshape(n_cols, n_rows), t


def organised_numpy(model, r, t, gate=None):
    """the header's model on the host: (xyz [n, 3] f32 with NaN where invalid, valid [n])"""
    x1, y1, z1, x2, y2, z2 = model
    n_cols, n_rows = r.shape
    rm = r.astype(np.float32) * np.float32(0.001)
    valid = (r != 0) & np.isfinite(t)[:, None]
    if gate is not None:
        if gate.row_step > 1:
            valid &= (np.arange(n_rows) % gate.row_step == 0)[None, :]
        if gate.use_range:
            valid &= (np.float32(gate.range_min) <= rm) & (rm <= np.float32(gate.range_max))
    xyz = np.stack([fma_f32(rm, d, o[:, None]) for d, o in ((x1, x2), (y1, y2), (z1, z2))], 2)
    xyz[~valid] = np.nan
    return xyz.reshape(-1, 3), valid.ravel()


def device_unproject(ndt, hipmem, r, refl, t, traj=None, ref=None, gate=None, filt=None, cap=None, alloc=None, fill=None,
                     want_intensity=True):
    """ndt_unproject_device on uploaded arrays -> dict(xyz [m, 3], intensity, t, index, m); the whole output arrays as
    downloaded are kept in device_unproject.last_raw.  alloc: elements the output arrays hold (default: cap)."""
    n = r.size
    cap = n if cap is None else cap
    alloc = cap if alloc is None else alloc
    d_r, d_t = hipmem.upload(r.ravel()), hipmem.upload(t)
    d_refl = None if refl is None else hipmem.upload(refl.ravel())
    init = np.full(max(alloc, 1), np.nan if fill is None else fill, np.float32)
    dout = [hipmem.upload(init) for _ in range(3)]
    doi = hipmem.upload(init) if (refl is not None and want_intensity) else None
    dot = hipmem.upload(init)
    didx = hipmem.upload(np.full(max(alloc, 1), -7, np.int32))
    kt, kp = (None, None) if traj is None else traj
    try:
        m = ndt.unprojectDevice(d_r, d_refl, d_t, dout[0], dout[1], dout[2], cap, knot_t=kt, knot_poses=kp, ref_pose=ref, gate=gate,
                                filter=filt, o_intensity=doi, o_t=dot, d_index=didx)
    finally:
        raw = dict(xyz=np.stack([download(hipmem, p, alloc) for p in dout], 1),
                   intensity=None if doi is None else download(hipmem, doi, alloc), t=download(hipmem, dot, alloc),
                   index=download(hipmem, didx, alloc, np.int32))
        device_unproject.last_raw = raw
    return dict(xyz=raw["xyz"][:m], intensity=None if doi is None else raw["intensity"][:m], t=raw["t"][:m], index=raw["index"][:m], m=m)


# ---- 1. the organised form, no trajectory: the exact fused multiply-add -------------------------------------------------
def test_the_host_fma_is_exact():
    """fma_f32 against fractions.Fraction: random operands, and sums that land on the midpoint of two floats"""
    rng = np.random.default_rng(1)
    a = (rng.integers(0, 2 ** 20, 3000).astype(np.float32) * np.float32(0.001))
    b = rng.uniform(-1.0, 1.0, 3000).astype(np.float32)
    c = rng.uniform(-0.05, 0.05, 3000).astype(np.float32)
    # sums that float64 puts exactly ON the midpoint of two floats although the exact value lies beside it:
    # 4097 * 4097 = 2^24 + 2^13 + 1 (float spacing 2 there), +2^-40 is lost in float64 -- the exact sum rounds UP, the
    # float64 sum to even, down; 4097 * 4099 = 2^24 + 2^14 + 3, -2^-40: the exact sum rounds DOWN, the float64 sum to even, up
    a[:2], b[:2], c[:2] = [4097.0, 4097.0], [4097.0, 4099.0], [2.0 ** -40, -2.0 ** -40]
    got = fma_f32(a, b, c)
    want = np.array([fma_fraction(*v) for v in zip(a, b, c)], np.float32)
    assert np.array_equal(bits(got), bits(want))
    assert got[0] == 2 ** 24 + 2 ** 13 + 2 and got[1] == 2 ** 24 + 2 ** 14 + 2
    plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert plain[0] != got[0] and plain[1] != got[1]      # (what the correction is for)


@pytest.mark.parametrize("n_cols,n_rows", ORGANISED_SHAPES)
def test_organised_form_is_the_exact_fma(pkg, ndt, hipmem, n_cols, n_rows):
    try:
        n = n_cols * n_rows
        model = random_model(n_cols, n_rows, 10 + n)
        ndt.setScanModel(*model)
        assert ndt.scanModelInfo() == (n_cols, n_rows)
        images = [random_image(n_cols, n_rows, 20 + n)]
        if n < len(SPECIAL_RANGES):                       # too few pixels for every special range in one image
            images = [(np.full((n_cols, n_rows), v, np.uint32), images[0][1], np.zeros(n_cols, np.float32)) for v in SPECIAL_RANGES]
        for r, refl, t in images:
            # the vectorised reference against Fraction, every pixel of these small shapes
            rm = r.astype(np.float32) * np.float32(0.001)
            for d, o in ((model[0], model[3]), (model[1], model[4]), (model[2], model[5])):
                want = [fma_fraction(rm[c, k], d[c, k], o[c]) for c in range(n_cols) for k in range(n_rows)]
                assert np.array_equal(bits(fma_f32(rm, d, o[:, None]).ravel()), bits(np.array(want, np.float32)))
            rm_live = np.sort(np.unique(rm[(r != 0) & np.isfinite(t)[:, None]]))
            gates = [None, pkg.RangeGate(), pkg.RangeGate(row_step=1), pkg.RangeGate(row_step=2), pkg.RangeGate(row_step=3),
                     pkg.RangeGate(0.0, 2000.0), pkg.RangeGate(None, 100.0, row_step=2)]
            if len(rm_live):
                # bounds hit exactly by a pixel on either side: both pixels must come out (inclusive)
                lo, hi = rm_live[len(rm_live) // 4], rm_live[(3 * len(rm_live)) // 4]
                gates += [pkg.RangeGate(float(lo), float(hi)), pkg.RangeGate(float(lo), float(lo), row_step=1)]
            for gate in gates:
                want, valid = organised_numpy(model, r, t, gate)
                if gate is not None and gate.use_range and gate.range_min == gate.range_max and gate.range_min > 0:
                    assert valid.any() and (valid.sum() < max(2, (r != 0).sum()))
                got = device_unproject(ndt, hipmem, r, refl, t, gate=gate, fill=-1.0)
                what = (n_cols, n_rows, None if gate is None else (gate.use_range, gate.range_min, gate.range_max, gate.row_step))
                assert got["m"] == n, what
                assert np.array_equal(np.isnan(got["xyz"]), np.isnan(want)), what          # NaN exactly where invalid
                assert np.array_equal(np.isnan(got["xyz"]).all(1), ~valid), what
                assert np.array_equal(bits(got["xyz"]), bits(want)), what                  # (one NaN pattern: the default quiet NaN)
                assert np.array_equal(got["intensity"], refl.ravel().astype(np.float32)), what
                assert np.array_equal(bits(got["t"]), bits(np.repeat(t, n_rows))), what
                assert np.array_equal(got["index"], np.arange(n)), what
                hipmem.free_all()
            # without a reflectivity array and without the optional outputs
            d_r, d_t = hipmem.upload(r.ravel()), hipmem.upload(t)
            o = [hipmem.upload(np.full(n, -1.0, np.float32)) for _ in range(3)]
            assert ndt.unprojectDevice(d_r, None, d_t, o[0], o[1], o[2], n) == n
            want, _ = organised_numpy(model, r, t)
            assert np.array_equal(bits(np.stack([download(hipmem, p, n) for p in o], 1)), bits(want))
            hipmem.free_all()
    except BaseException:
        STATE["organised_failed"] = True
        raise


# ---- 2. fused equals composed ---------------------------------------------------------------------------------------------
def filters(pkg):
    return [("none", None, True), ("zeroed", pkg.ScanFilter(), True),
            ("box", pkg.ScanFilter.from_vehicle_box([100.0, -50.0, 0.0], [400.0, 500.0, 600.0]), True),
            ("z or intensity", pkg.ScanFilter.from_vehicle_box(None, None, z_band=(-300.0, 50.0), intensity_keep_min=128.0), True),
            ("z or intensity, no reflectivity", pkg.ScanFilter.from_vehicle_box(None, None, z_band=(-300.0, 50.0), intensity_keep_min=128.0), False),
            ("all", pkg.ScanFilter.from_vehicle_box([0.0, 0.0, 0.0], [700.0, 700.0, 700.0], z_band=(-500.0, 100.0), intensity_keep_min=200.0), True)]


@pytest.mark.parametrize("n_knots", [0, 1, 2, 5, 64])
def test_fused_equals_composed(pkg, ndt, hipmem, n_knots):
    """xyz, intensity, t, index and n_out of the fused call are bit for bit what ndt_deskew_device returns for the organised
    output of test 1 (n_knots = 0: no trajectory -- the filter alone, against the boolean mask of that output)"""
    if STATE["organised_failed"]:
        pytest.skip("the organised form failed: there is nothing to compose")
    for n_cols, n_rows in ((3, 85), (257, 1), (5, 205)):
        n = n_cols * n_rows
        ndt.setScanModel(*random_model(n_cols, n_rows, 40 + n))
        if n_knots:
            kt, kp = make_trajectory(n_knots, 70 + n_knots)
            if n_knots == 5:
                kp[2] = kp[1]                                        # a rigid segment
            kt = f32_knots(kt)
            refs = ref_choices(kp, n_knots)
        else:
            kt, kp, refs = np.array([0.0, 1.0]), None, [("none", None)]
        span = float(kt[-1]) if kt[-1] > 0 else 1.0
        r, refl, t = random_image(n_cols, n_rows, 50 + n + n_knots, span=span)
        gate = pkg.RangeGate(0.5, 900.0, row_step=2 if n_rows > 1 else 0)
        org = device_unproject(ndt, hipmem, r, refl, t, gate=gate)
        hipmem.free_all()
        if n_cols > 100:                                             # times outside the knots on either side
            assert (t[np.isfinite(t)] < kt[0]).any() and (t[np.isfinite(t)] > kt[-1]).any()
        for rname, ref in refs:
            for fname, filt, with_refl in filters(pkg):
                inten = org["intensity"] if with_refl else None
                what = (n_cols, n_rows, n_knots, rname, fname)
                fused = device_unproject(ndt, hipmem, r, refl if with_refl else None, t, traj=(kt, kp) if n_knots else None, ref=ref,
                                         gate=gate, filt=filt, fill=-1.0)
                if n_knots:
                    xyz, oi, idx, m = device_deskew(ndt, hipmem, org["xyz"], org["t"], kt, kp, ref=ref, filt=filt, inten=inten)
                else:
                    sel = np.arange(n) if filt is None else np.flatnonzero(keep_numpy(filt, org["xyz"], org["t"], inten))
                    xyz, oi, idx, m = org["xyz"][sel], None if inten is None else inten[sel], sel, len(sel)
                assert fused["m"] == m and (0 < m < n if filt is not None else m == n), what + (m,)
                assert np.array_equal(bits(fused["xyz"]), bits(xyz)), what
                assert np.array_equal(fused["index"], idx), what
                assert np.array_equal(bits(fused["t"]), bits(org["t"][idx])), what
                if with_refl:
                    assert np.array_equal(bits(fused["intensity"]), bits(oi)), what
                if filt is not None:                                 # nothing behind the kept points
                    raw = device_unproject.last_raw
                    assert np.all(raw["xyz"][m:] == -1.0) and np.all(raw["t"][m:] == -1.0) and np.all(raw["index"][m:] == -7), what
                hipmem.free_all()


# ---- 3. compaction boundaries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols,n_rows", COMPACT_SHAPES)
def test_compaction_boundaries(pkg, ndt, hipmem, n_cols, n_rows):
    n = n_cols * n_rows
    model = random_model(n_cols, n_rows, 3)
    ndt.setScanModel(*model)
    kt, kp = make_trajectory(3, 33)
    kt = f32_knots(kt)
    r, refl, t = random_image(n_cols, n_rows, n % 1000, zero_share=0.0, nan_cols=False, span=float(kt[-1]))
    r[r == 0] = 7                                                    # (the special range 0: every pixel valid here)
    half_r = r.copy()
    half_r[np.random.default_rng(n).uniform(size=r.shape) < 0.25] = 0
    everything = pkg.ScanFilter.from_vehicle_box([0.0, 0.0, 0.0], [4000.0, 4000.0, 4000.0])
    upper = pkg.ScanFilter.from_vehicle_box(None, None, z_band=(-2000.0, 100.0))        # z <= 100 m: about two thirds
    moved = device_unproject(ndt, hipmem, r, refl, t, traj=(kt, kp))                     # what the emit must write
    hipmem.free_all()
    for name, image, filt in (("all", r, pkg.ScanFilter()), ("none", r, everything), ("half", half_r, upper)):
        raw_pts, valid = organised_numpy(model, image, t)
        keep = keep_numpy(filt, raw_pts, np.repeat(t, n_rows), refl.ravel().astype(np.float32))
        sel = np.flatnonzero(keep)
        assert {"all": len(sel) == n, "none": len(sel) == 0, "half": 0.4 * n <= len(sel) <= 0.6 * n}[name], (name, len(sel))
        got = device_unproject(ndt, hipmem, image, refl, t, traj=(kt, kp), filt=filt, fill=-1.0)
        assert got["m"] == len(sel), (name, got["m"], len(sel))
        assert np.array_equal(got["index"], sel), name
        assert np.array_equal(bits(got["xyz"]), bits(moved["xyz"][sel])), name           # the same arithmetic as the organised launch
        assert np.array_equal(got["intensity"], refl.ravel()[sel].astype(np.float32)), name
        raw = device_unproject.last_raw
        assert np.all(raw["xyz"][got["m"]:] == -1.0) and np.all(raw["index"][got["m"]:] == -7), name
        hipmem.free_all()
        if name == "half":
            # too small a cap: n_out reported, the error returned, nothing beyond cap in arrays that are larger
            m, cap = len(sel), len(sel) - 3
            with pytest.raises(pkg.NdtError) as e:
                device_unproject(ndt, hipmem, image, refl, t, traj=(kt, kp), filt=filt, cap=cap, alloc=n, fill=-1.0)
            assert e.value.code == -1 and str(m) in str(e.value) and ndt.last_unproject_count == m
            raw = device_unproject.last_raw
            assert np.all(raw["xyz"][cap:] == -1.0) and np.all(raw["intensity"][cap:] == -1.0) and np.all(raw["t"][cap:] == -1.0)
            assert np.all(raw["index"][cap:] == -7)
            assert np.array_equal(bits(raw["xyz"][:cap]), bits(got["xyz"][:cap])) and np.array_equal(raw["index"][:cap], sel[:cap])
            hipmem.free_all()
    # the organised output of the whole image against the exact reference (no trajectory)
    got = device_unproject(ndt, hipmem, half_r, refl, t)
    want, _ = organised_numpy(model, half_r, t)
    assert np.array_equal(bits(got["xyz"]), bits(want))


# ---- 4. the three forms agree ---------------------------------------------------------------------------------------------
def test_host_form_equals_device_form(pkg, ndt, hipmem):
    n_cols, n_rows = 37, 70
    n = n_cols * n_rows
    ndt.setScanModel(*random_model(n_cols, n_rows, 91))
    kt, kp = make_trajectory(22, 61, [np.deg2rad(0.3), 1e-5, np.deg2rad(1.0)], trans=0.1)
    kt = f32_knots(kt)
    r, refl, t = random_image(n_cols, n_rows, 92, span=float(kt[-1]))
    gate = pkg.RangeGate(1.0, 800.0, row_step=3)
    f = pkg.ScanFilter.from_vehicle_box([0.0, 0.0, 0.0], [300.0, 300.0, 300.0], z_band=(-400.0, 100.0), intensity_keep_min=200.0)
    kt64, poses = np.ascontiguousarray(kt, np.float64), np.ascontiguousarray(np.transpose(kp, (0, 2, 1))).ravel()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    for traj in (None, (kt, kp)):
        for filt in (None, pkg.ScanFilter(), f):
            dev = device_unproject(ndt, hipmem, r, refl, t, traj=traj, gate=gate, filt=filt)
            m = dev["m"]
            assert m == n if filt is None else 0 < m < n
            kw = dict(knot_t=None if traj is None else kt, knot_poses=None if traj is None else kp, gate=gate, filter=filt)
            cloud, tt, idx = ndt.unproject(r, refl, t, with_t=True, with_index=True, **kw)
            assert cloud.shape == (m, 4) and np.array_equal(bits(cloud[:, :3]), bits(dev["xyz"]))
            assert np.array_equal(bits(cloud[:, 3]), bits(dev["intensity"]))
            assert np.array_equal(bits(tt), bits(dev["t"])) and np.array_equal(idx, dev["index"])
            plain = ndt.unproject(r, None, t, **kw)
            nodev = device_unproject(ndt, hipmem, r, None, t, traj=traj, gate=gate, filt=filt)
            assert plain.shape == (nodev["m"], 3) and np.array_equal(bits(plain), bits(nodev["xyz"]))
            # strided output through the C-ABI: pcl::PointXYZI (32 bytes, intensity at 16), 16 bytes without an intensity
            # slot, packed xyz
            for stride, off in ((32, 16), (16, -1), (12, -1), (20, 12)):
                out = np.full((n, stride // 4), -1.0, np.float32)
                n_out = C.c_size_t(0)
                g = C.byref(gate)
                rc = pkg.lib().ndt_unproject(ndt._h, r.ctypes.data, refl.ctypes.data, t.ctypes.data, g, *((None, None, 0) if traj is None
                                             else (dp(kt64), dp(poses), len(kt64))), None, None if filt is None else C.byref(filt),
                                             out.ctypes.data, stride, off, None, None, n, C.byref(n_out))
                assert rc == 0 and n_out.value == m, (stride, off, pkg.lib().ndt_last_error(ndt._h))
                assert np.array_equal(bits(out[:m, :3]), bits(dev["xyz"]))
                written = [0, 1, 2] + ([off // 4] if off >= 0 else [])
                if off >= 0:
                    assert np.array_equal(bits(out[:m, off // 4]), bits(dev["intensity"]))
                rest = [c for c in range(stride // 4) if c not in written]
                assert np.all(out[:m, rest] == -1.0) and np.all(out[m:] == -1.0)
            # the keyframe form: the archive read back through the source
            kept = ndt.putKeyframeFromRanges(5, r, refl, t, **kw)
            comp = dev if filt is not None else device_unproject(ndt, hipmem, r, refl, t, traj=traj, gate=gate, filt=pkg.ScanFilter())
            assert kept == comp["m"]
            ndt.setInputSourceFromKeyframe(5)
            back = read_source(pkg, ndt)
            assert back.shape == comp["xyz"].shape and np.array_equal(bits(back), bits(comp["xyz"]))
            # replacing the keyframe that is the viewed source unsets the source, as ndt_keyframe_put does
            assert ndt.putKeyframeFromRanges(5, r, refl, t, **kw) == kept
            assert ndt.sourceSize() == 0
            hipmem.free_all()
    # the archived scan feeds the map like any keyframe
    ndt.mapReset(1.0)
    ndt.mapAddKeyframe(5, np.eye(4))
    assert ndt.mapInfo()["n_points"] == kept
    ndt.mapClear()
    before = ndt.keyframeCount()
    ndt.eraseKeyframe(5)
    assert ndt.keyframeCount() == before - 1
    # host-form capacity: compacting reports the count, organised refuses before anything is written
    out, n_out = np.full((n, 3), -1.0, np.float32), C.c_size_t(0)
    rc = pkg.lib().ndt_unproject(ndt._h, r.ctypes.data, refl.ctypes.data, t.ctypes.data, None, None, None, 0, None, C.byref(f),
                                 out.ctypes.data, 12, -1, None, None, 5, C.byref(n_out))
    assert rc == -1 and n_out.value > 5 and str(n_out.value) in pkg.lib().ndt_last_error(ndt._h).decode() and np.all(out == -1.0)
    rc = pkg.lib().ndt_unproject(ndt._h, r.ctypes.data, refl.ctypes.data, t.ctypes.data, None, None, None, 0, None, None,
                                 out.ctypes.data, 12, -1, None, None, n - 1, C.byref(n_out))
    assert rc == -1 and n_out.value == n and np.all(out == -1.0)


# ---- 5. ground truth --------------------------------------------------------------------------------------------------------
def test_points_lie_on_the_surfaces_they_were_cast_at(pkg, S, ndt):
    """A range image of synth's analytic scene, 96 x 32, from a moving sensor, knots = the generating trajectory: every
    point of unproject + deskew within 0.5 mm (range quantisation) + 0.1 mm (f32 spacing at the scene's 60 m, 3.8e-6 m,
    times the handful of roundings) of its plane.  Without the trajectory at least half of the points violate that bound
    (the generator's own check on the host, tests/test_unproject_cpu.py, has 99 %)."""
    c = moving_scene(pkg, S, no_return=0.1, drop_columns=3)
    img = c["img"]
    ndt.setScanModel(*c["model"])
    live = ((img["surface"] >= 0) & np.isfinite(img["col_t"])[:, None]).ravel()
    surface = img["surface"].ravel()
    for filt in (None, pkg.ScanFilter()):
        cloud, idx = ndt.unproject(img["range_mm"], img["reflectivity"], img["col_t"], c["kt"], c["kp"], filter=filt, with_index=True)
        assert np.array_equal(idx, np.arange(live.size) if filt is None else np.flatnonzero(live))
        assert np.array_equal(np.isfinite(cloud[:, :3]).all(1), live[idx])
        d = surface_distance(cloud[:, :3], c["ref"], surface[idx], img["planes"])
        print("deskewed: %d points, worst %.3e m" % (live.sum(), np.nanmax(d[live[idx]])))
        assert np.nanmax(d[live[idx]]) <= SURFACE_BOUND
    raw = ndt.unproject(img["range_mm"], img["reflectivity"], img["col_t"])
    d = surface_distance(raw[:, :3], c["ref"], surface, img["planes"])
    share = float((d[live] > SURFACE_BOUND).mean())
    print("without the trajectory: %.1f %% beyond the bound, worst %.3f m" % (100.0 * share, np.nanmax(d[live])))
    assert share >= 0.5
    # the scene through the archive: deskewed, registered against itself at the identity
    assert ndt.putKeyframeFromRanges(31, img["range_mm"], img["reflectivity"], img["col_t"], c["kt"], c["kp"]) == live.sum()
    ndt.eraseKeyframe(31)


# ---- 6. refusals and state ----------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_name_the_cause(pkg, ndt, hipmem):
    n_cols, n_rows = 6, 50
    n = n_cols * n_rows
    model = random_model(n_cols, n_rows, 5)
    r, refl, t = random_image(n_cols, n_rows, 6)
    kt, kp = make_trajectory(3, 8)
    d_r, d_refl, d_t = hipmem.upload(r.ravel()), hipmem.upload(refl.ravel()), hipmem.upload(t)
    outs = [hipmem.upload(np.full(n, -1.0, np.float32)) for _ in range(5)]
    d_idx = hipmem.upload(np.full(n, -7, np.int32))
    f = pkg.ScanFilter()

    def refused(cause, rng=d_r, rf=d_refl, ct=d_t, o=None, cap=n, **kw):
        o = outs if o is None else o
        with pytest.raises(pkg.NdtError) as e:
            ndt.unprojectDevice(rng, rf, ct, o[0], o[1], o[2], cap, o_intensity=o[3], o_t=o[4], d_index=d_idx, **kw)
        assert e.value.code == -1 and cause in str(e.value), (cause, str(e.value))
        assert all(np.all(download(hipmem, p, n) == -1.0) for p in outs) and np.all(download(hipmem, d_idx, n, np.int32) == -7), cause
        assert np.array_equal(download(hipmem, d_r, n, np.uint32), r.ravel()) and np.array_equal(download(hipmem, d_t, n_cols), t, equal_nan=True)

    ndt.clearScanModel()
    assert ndt.scanModelInfo() == (0, 0)
    refused("no scan model")
    refused("no scan model", filter=f)
    with pytest.raises(pkg.NdtError) as e:
        ndt.unproject(r, refl, t)
    assert "no scan model" in str(e.value)
    archived = ndt.keyframeCount()
    with pytest.raises(pkg.NdtError):
        ndt.putKeyframeFromRanges(990, r, refl, t)
    assert ndt.keyframeCount() == archived
    # set twice with different shapes: the second holds
    ndt.setScanModel(*random_model(9, 11, 1))
    assert ndt.scanModelInfo() == (9, 11)
    ndt.setScanModel(*model)
    assert ndt.scanModelInfo() == (n_cols, n_rows)
    got = device_unproject(ndt, hipmem, r, refl, t)
    assert np.array_equal(bits(got["xyz"]), bits(organised_numpy(model, r, t)[0]))
    for filt in (None, f):
        refused("NULL", rng=None, filter=filt)
        refused("NULL", ct=None, filter=filt)
        for k in range(3):
            refused("NULL", o=[None if j == k else p for j, p in enumerate(outs)], filter=filt)
        refused("reflectivity", rf=None, filter=filt)                     # an intensity output without the input
        # output / input overlap: an output inside the range image, on its last byte, on the column times, on the reflectivity
        for bad in (d_r, d_r + 4 * n - 4, d_t, d_refl + n - 1):
            for k in range(5):
                refused("overlap", o=[bad if j == k else p for j, p in enumerate(outs)], filter=filt)
        refused("row_step", gate=pkg.RangeGate(row_step=-1), filter=filt)
        refused("range_min", gate=pkg.RangeGate(2.0, 1.0), filter=filt)
        refused("range_min", gate=pkg.RangeGate(np.nan, 1.0), filter=filt)
        refused("strictly increasing", knot_t=kt[::-1].copy(), knot_poses=kp, filter=filt)
        refused("non-finite knot time", knot_t=[0.0, np.nan, 1.0], knot_poses=kp, filter=filt)
        bad_pose = kp.copy()
        bad_pose[1, 0, 3] = np.inf
        refused("non-finite pose entry", knot_t=kt, knot_poses=bad_pose, filter=filt)
        # two outputs that are one array, or overlap
        refused("overlap", o=[outs[0], outs[0]] + outs[2:], filter=filt)
        refused("overlap", o=outs[:4] + [outs[1] + 4 * n - 4], filter=filt)
    L = pkg.lib()
    n_out = C.c_size_t(99)
    args = (d_r, d_refl, d_t, None)
    tail = (None, outs[0], outs[1], outs[2], None, None, None, n, C.byref(n_out))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    kt64, poses = np.ascontiguousarray(kt), np.ascontiguousarray(np.transpose(kp, (0, 2, 1))).ravel()
    last_error = lambda: L.ndt_last_error(ndt._h).decode()   # noqa: E731
    assert L.ndt_unproject_device(ndt._h, *args, dp(kt64), dp(poses), 0, None, *tail) == -1      # knots given, n_knots = 0
    assert "n_knots outside" in last_error()
    assert L.ndt_unproject_device(ndt._h, *args, dp(kt64), dp(poses), 65, None, *tail) == -1
    assert "n_knots outside" in last_error()
    assert L.ndt_unproject_device(ndt._h, *args, None, dp(poses), 3, None, *tail) == -1
    assert "null pointer" in last_error()
    assert L.ndt_unproject_device(ndt._h, *args, dp(kt64), dp(poses), 3, None, None, outs[0], outs[1], outs[2], None, None, None, n, None) == -1
    assert "n_out" in L.ndt_last_error(ndt._h).decode()
    assert L.ndt_unproject_device(None, *args, None, None, 0, None, *tail) == -1
    assert all(np.all(download(hipmem, p, n) == -1.0) for p in outs)
    # the host and keyframe forms: each NULL named, the output cloud and the archive untouched
    cloud, archived = np.full((n, 3), -1.0, np.float32), ndt.keyframeCount()
    host_tail = (None, None, None, 0, None, None)
    for rng, ct, out, cause in ((None, t, cloud, "range image"), (r, None, cloud, "column times"), (r, t, None, "output cloud")):
        rc = L.ndt_unproject(ndt._h, None if rng is None else rng.ctypes.data, refl.ctypes.data, None if ct is None else ct.ctypes.data,
                             *host_tail, None if out is None else out.ctypes.data, 12, -1, None, None, n, C.byref(n_out))
        assert rc == -1 and "NULL" in last_error() and cause in last_error(), (cause, last_error())
    rc = L.ndt_unproject(ndt._h, r.ctypes.data, None, t.ctypes.data, *host_tail, cloud.ctypes.data, 16, 12, None, None, n, C.byref(n_out))
    assert rc == -1 and "reflectivity" in last_error()                   # an intensity slot without the input
    rc = L.ndt_unproject(ndt._h, r.ctypes.data, refl.ctypes.data, t.ctypes.data, *host_tail, cloud.ctypes.data, 10, -1, None, None, n, C.byref(n_out))
    assert rc == -1 and "layout" in last_error()
    for rng, ct in ((None, t), (r, None)):
        rc = L.ndt_keyframe_put_from_ranges(ndt._h, 992, None if rng is None else rng.ctypes.data, refl.ctypes.data,
                                            None if ct is None else ct.ctypes.data, *host_tail, None)
        assert rc == -1 and "NULL" in last_error()
    assert np.all(cloud == -1.0) and ndt.keyframeCount() == archived
    # organised: cap below the pixel count -- refused before anything is written, *n_out = the pixel count
    refused(str(n), cap=n - 1)
    assert ndt.last_unproject_count == n
    # ... and the same call with nothing wrong goes through
    assert ndt.unprojectDevice(d_r, d_refl, d_t, outs[0], outs[1], outs[2], n, o_intensity=outs[3], o_t=outs[4], d_index=d_idx) == n
    for p in outs:                                                       # (the sentinels again, for the refusals below)
        hipmem.write(p, np.full(n, -1.0, np.float32))
    hipmem.write(d_idx, np.full(n, -7, np.int32))
    # the model's own refusals keep the model that is set
    x1, y1, z1, x2, y2, z2 = model
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    for bad in ((0, n_rows), (n_cols, 0), (-1, 1), (65536, 32768)):
        assert L.ndt_scan_model_set(ndt._h, bad[0], bad[1], fp(x1), fp(y1), fp(z1), fp(x2), fp(y2), fp(z2)) == -1
    assert L.ndt_scan_model_set(ndt._h, n_cols, n_rows, fp(x1), None, fp(z1), fp(x2), fp(y2), fp(z2)) == -1
    assert ndt.scanModelInfo() == (n_cols, n_rows)
    ndt.clearScanModel()
    refused("no scan model")


def test_unproject_leaves_the_engine_state_alone(pkg, S, ndt, hipmem):
    cfg = S.config_c1(max_points=4000)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    ndt.mapReset(1.0)
    ndt.mapAdd(cfg["target"][:500])
    ndt.putKeyframe(70, cfg["source"][:300])
    T1 = ndt.align(cfg["guess"])
    hist1, leaves1, src1, map1, kf1 = ndt.getIterationHistory(), ndt.getLeaves(), read_source(pkg, ndt), ndt.mapInfo(), ndt.keyframeCount()
    counters = lambda: (ndt.prelaunchCounters(), ndt.speculationCounters(), ndt.buildCounters(), ndt.handoffCounters(),   # noqa: E731
                        ndt.getTiming()["n_eval_launches"], ndt.getResult()["n_evaluations"])
    counters1 = counters()
    export1 = ndt.mapExport()
    n_cols, n_rows = 40, 64
    ndt.setScanModel(*random_model(n_cols, n_rows, 2))
    kt, kp = make_trajectory(5, 13)
    r, refl, t = random_image(n_cols, n_rows, 14, span=float(kt[-1]))
    ndt.unproject(r, refl, t)
    ndt.unproject(r, refl, t, kt, kp, filter=pkg.ScanFilter(), gate=pkg.RangeGate(1.0, 500.0, row_step=2))
    device_unproject(ndt, hipmem, r, refl, t, traj=(kt, kp), filt=pkg.ScanFilter())
    device_unproject(ndt, hipmem, r, None, t)
    with pytest.raises(pkg.NdtError):
        ndt.unproject(r, refl, t, kt[::-1].copy(), kp)
    ndt.clearScanModel()
    hist2, leaves2 = ndt.getIterationHistory(), ndt.getLeaves()
    assert counters() == counters1
    for a, b in zip(hist1, hist2):
        assert a.tobytes() == b.tobytes()
    assert sorted(leaves1) == sorted(leaves2)
    for k in leaves1:
        assert np.asarray(leaves1[k]).tobytes() == np.asarray(leaves2[k]).tobytes(), k
    assert read_source(pkg, ndt).tobytes() == src1.tobytes()
    assert ndt.mapInfo() == map1 and ndt.keyframeCount() == kf1 and np.asarray(ndt.mapExport()).tobytes() == np.asarray(export1).tobytes()
    T2 = ndt.align(cfg["guess"])
    assert T1.tobytes() == T2.tobytes()
    for a, b in zip(hist1, ndt.getIterationHistory()):
        assert a.tobytes() == b.tobytes()
    ndt.setInputSourceFromKeyframe(70)                                   # the archive still holds what was put
    assert np.array_equal(read_source(pkg, ndt), cfg["source"][:300].astype(np.float32))
    ndt.eraseKeyframe(70)
    ndt.mapClear()


# ---- 7. the C++ face ------------------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, tmp_path):
    """tests/cpp/test_unproject.cpp against the API mocks, built with the g++ line tests/test_gpu_deskew.py uses."""
    d = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "test_unproject")
    lib = os.path.join(ROOT, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(ROOT, "include", "compat"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(d, "test_unproject.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "unproject: PASS" in p.stdout
