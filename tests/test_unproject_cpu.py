"""The scan model on the host: ndt_scan_model_from_beams against a NumPy restatement of the lidar callback's formula with
float64 angles, its refusals, that host code under AddressSanitizer + UBSan as a stand-alone program, the seeded
range-image generator of synth.py against its own analytic scene, and the unprojection kernels' scratch use.  No GPU.
The helpers are shared with tests/test_gpu_unproject.py.

Bound of the table comparison: a direction component may differ by at most 2e-6 -- the float angle, up to 2 pi, carries
half an ulp of 4.8e-7 twice (the degree-to-radian product and the sum of the two azimuths), sinf / cosf add 1 ulp
(6e-8) and the two products their roundings: below 1e-6, doubled.  An offset component by at most 1e-7 m: the angle's
error times the 27 mm lever (1.4e-8 m) plus the one float rounding of a value below 1 m (3e-8 m)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
SHAPES = [(1, 1), (7, 3), (2048, 128)]
SURFACE_BOUND = 0.5e-3 + 0.1e-3      # range quantisation + f32 spacing at the scene's 60 m (3.8e-6 m) times a handful of roundings


def beams():
    with open(os.path.join(ROOT, "tests", "golden", "os2_128_beams.json")) as f:
        return json.load(f)


def beam_angles(n_rows):
    """the first n_rows rows of the OS2-128's angles (degrees) and its beam origin (mm)"""
    b = beams()
    assert len(b["beam_azimuth_angles"]) == len(b["beam_altitude_angles"]) == b["pixels_per_column"] == 128
    return (np.array(b["beam_azimuth_angles"][:n_rows], np.float32), np.array(b["beam_altitude_angles"][:n_rows], np.float32),
            float(b["lidar_origin_to_beam_origin_mm"]))


def lidar_to_body_choices(S):
    """the identity and a mounting with every rotation axis and every translation in play (below 1 m per axis)"""
    return [("identity", np.eye(4)), ("mounted", S.pose_matrix(0.31, -0.22, 0.47, 0.02, -0.035, 2.4))]


def tables_numpy(n_cols, az_deg, alt_deg, origin_mm, T):
    """the formula of the lidar callback's Initialize() in float64 throughout: (d [n_cols, n_rows, 3], o [n_cols, 3])"""
    az = np.deg2rad(np.asarray(az_deg, np.float32).astype(np.float64))
    alt = np.deg2rad(np.asarray(alt_deg, np.float32).astype(np.float64))
    meas = 2.0 * np.pi * (1.0 - np.arange(n_cols, dtype=np.float64) / n_cols)
    total = meas[:, None] + az[None, :]
    d = np.stack([np.cos(alt) * np.cos(total), np.cos(alt) * np.sin(total), np.broadcast_to(np.sin(alt), total.shape)], 2)
    r0 = origin_mm * 1e-3
    o = np.stack([r0 * np.cos(meas), r0 * np.sin(meas), np.zeros(n_cols)], 1)
    return d @ T[:3, :3].T, o @ T[:3, :3].T + T[:3, 3]


@pytest.mark.parametrize("n_cols,n_rows", SHAPES)
def test_tables_match_the_float64_restatement(pkg, S, n_cols, n_rows):
    az, alt, mm = beam_angles(n_rows)
    for name, T in lidar_to_body_choices(S):
        x1, y1, z1, x2, y2, z2 = pkg.scan_model_from_beams(n_cols, az, alt, mm, T)
        assert x1.shape == y1.shape == z1.shape == (n_cols, n_rows) and x2.shape == y2.shape == z2.shape == (n_cols,)
        assert all(a.dtype == np.float32 for a in (x1, y1, z1, x2, y2, z2))
        d, o = tables_numpy(n_cols, az, alt, mm, T)
        err_d = np.abs(np.stack([x1, y1, z1], 2).astype(np.float64) - d).max()
        err_o = np.abs(np.stack([x2, y2, z2], 1).astype(np.float64) - o).max()
        print("%d x %d, %s: directions %.3e, offsets %.3e m" % (n_cols, n_rows, name, err_d, err_o))
        assert err_d <= 2e-6, (name, err_d)
        assert err_o <= 1e-7, (name, err_o)
    # None is the identity
    for a, b in zip(pkg.scan_model_from_beams(n_cols, az, alt, mm), pkg.scan_model_from_beams(n_cols, az, alt, mm, np.eye(4))):
        assert a.tobytes() == b.tobytes()


def test_tables_are_unit_directions_on_a_circle_of_offsets(pkg):
    az, alt, mm = beam_angles(128)
    x1, y1, z1, x2, y2, z2 = pkg.scan_model_from_beams(2048, az, alt, mm)
    norm = np.sqrt(x1.astype(np.float64) ** 2 + y1.astype(np.float64) ** 2 + z1.astype(np.float64) ** 2)
    assert np.abs(norm - 1.0).max() <= 4e-7                       # three float roundings of components below 1
    assert np.abs(np.hypot(x2.astype(np.float64), y2.astype(np.float64)) - mm * 1e-3).max() <= 1e-8 and not z2.any()
    # column 0 looks along +x (azimuth 2 pi), the columns turn clockwise seen from above
    assert x2[0] > 0.027 and abs(y2[0]) < 1e-6 and y2[512] < -0.027


def test_from_beams_refusals(pkg):
    L = pkg.lib()
    az, alt, mm = beam_angles(3)
    T = np.ascontiguousarray(np.eye(4).ravel())
    outs = [np.full(7 * 3, -1.0, np.float32) for _ in range(3)] + [np.full(7, -1.0, np.float32) for _ in range(3)]
    fp, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))

    def call(n_cols=7, n_rows=3, a=az, b=alt, origin=mm, t=T, skip=None):
        o = [None if k == skip else fp(v) for k, v in enumerate(outs)]
        return L.ndt_scan_model_from_beams(n_cols, n_rows, None if a is None else fp(a), None if b is None else fp(b), origin,
                                           None if t is None else dp(t), *o)

    assert call(a=None) == INVALID_ARG and call(b=None) == INVALID_ARG and call(t=None) == INVALID_ARG
    for k in range(6):
        assert call(skip=k) == INVALID_ARG
    for bad in ((0, 3), (7, 0), (-1, 3), (7, -2), (65536, 32768)):           # below 1, and 2^31 pixels
        assert call(n_cols=bad[0], n_rows=bad[1]) == INVALID_ARG
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            a = az.copy()
            a[k] = bad
            assert call(a=a) == INVALID_ARG and call(b=a) == INVALID_ARG
        assert call(origin=bad) == INVALID_ARG
        for e in (0, 5, 10, 12, 15):
            t = T.copy()
            t[e] = bad
            assert call(t=t) == INVALID_ARG
    assert all(np.all(v == -1.0) for v in outs)                              # refused: nothing written
    assert call() == 0 and not any(np.any(v == -1.0) for v in outs)
    with pytest.raises(pkg.NdtError):
        pkg.scan_model_from_beams(0, az, alt, mm)
    with pytest.raises(ValueError):
        pkg.scan_model_from_beams(7, az, alt[:2], mm)


def test_range_gate_struct(pkg):
    assert C.sizeof(pkg.RangeGate) == 16      # int, 2 floats, int: the struct of include/ndt_hip.h
    g = pkg.RangeGate()
    assert bytes(g) == bytes(16)
    g = pkg.RangeGate(0.5, 120.0, row_step=2)
    assert (g.use_range, g.range_min, g.range_max, g.row_step) == (1, 0.5, 120.0, 2)


# --------------------------------------------------------------------------- the range-image generator
def moving_scene(pkg, S, n_cols=96, n_rows=32, seed=5, **kw):
    """A range image of synth's analytic scene from a sensor that moves 1.2 m and yaws 4 degrees during the scan: the
    model, the image, the trajectory (5 knots) and the reference pose (the last knot)."""
    az, alt, mm = beam_angles(128)
    rows = np.linspace(0, 127, n_rows).astype(int)
    model = pkg.scan_model_from_beams(n_cols, az[rows], alt[rows], mm, S.pose_matrix(0.1, 0.0, 0.3, 0.0, 0.0, 0.0))
    kt = np.linspace(0.0, 0.1, 5)
    kp = np.stack([S.pose_matrix(2.0 + 12.0 * t, -3.0 + 2.0 * t, 2.0 + 0.5 * t, 0.2 * t, -0.1 * t, 0.3 + np.deg2rad(40.0) * t) for t in kt])
    col_t = np.linspace(0.0, 0.1, n_cols, endpoint=False).astype(np.float32)
    img = S.range_image(model, kt, kp, col_t, seed=seed, **kw)
    return dict(model=model, img=img, kt=kt, kp=kp, ref=kp[-1])


def surface_distance(points_ref, ref, surface, planes):
    """|normal . w - offset| of every point (given in the frame `ref`) to the plane it was cast at; NaN where none"""
    w = points_ref.astype(np.float64) @ ref[:3, :3].T + ref[:3, 3]
    out = np.full(surface.shape, np.nan)
    for s, (normal, offset) in enumerate(planes):
        m = surface == s
        out[m] = np.abs(w[m] @ np.asarray(normal, np.float64) - offset)
    return out


def test_generator_stays_on_its_surfaces(pkg, S):
    """the float64 unprojection + deskew of the generator's own image lies on the planes within the quantisation; the same
    image without the trajectory does not -- for at least half of the points"""
    c = moving_scene(pkg, S, no_return=0.1, drop_columns=3)
    img = c["img"]
    assert img["range_mm"].dtype == np.uint32 and img["reflectivity"].dtype == np.uint8 and img["col_t"].dtype == np.float32
    assert img["range_mm"].shape == img["surface"].shape == (96, 32) and len(img["dropped"]) == 3
    assert np.isnan(img["col_t"][img["dropped"]]).all() and np.isfinite(img["col_t"]).sum() == 93
    assert (img["range_mm"][img["dropped"]] > 0).any()                       # the time alone marks a dropped column
    assert np.array_equal(img["surface"] >= 0, img["range_mm"] > 0)
    hit = img["surface"] >= 0
    assert 0.4 < hit.mean() < 0.95 and all((img["surface"] == s).sum() > 50 for s in range(3)), hit.mean()
    assert 0.05 < (~hit).mean()
    live = hit & np.isfinite(img["col_t"])[:, None]
    moved = S.unproject_numpy(c["model"], img["range_mm"], img["col_t"], c["kt"], c["kp"])
    assert np.array_equal(np.isfinite(moved).all(2), live)
    d = surface_distance(moved, c["ref"], img["surface"], img["planes"])
    print("deskewed: worst %.3e m" % np.nanmax(d[live]))
    assert np.nanmax(d[live]) <= SURFACE_BOUND
    raw = S.unproject_numpy(c["model"], img["range_mm"], img["col_t"])
    d = surface_distance(raw, c["ref"], img["surface"], img["planes"])
    print("raw: %.1f %% beyond the bound, worst %.3f m" % (100.0 * (d[live] > SURFACE_BOUND).mean(), np.nanmax(d[live])))
    assert (d[live] > SURFACE_BOUND).mean() >= 0.5
    # seeded: the same call gives the same image, another seed another
    again = moving_scene(pkg, S, no_return=0.1, drop_columns=3)["img"]
    assert all(np.array_equal(img[k], again[k], equal_nan=True) for k in ("range_mm", "reflectivity", "col_t", "surface"))
    other = moving_scene(pkg, S, seed=6, no_return=0.1, drop_columns=3)["img"]
    assert not np.array_equal(img["reflectivity"], other["reflectivity"])


# --------------------------------------------------------------------------- sanitizers, stand-alone
def test_scan_model_host_code_under_asan_ubsan(tmp_path):
    """tests/cpp/sanitize_scan_model.cpp (its own main) + csrc/ndt_scan_model.cpp under ASan + UBSan as a child process: the
    tables written into buffers of exactly their size at the shapes above, plus the refusals.  Never through Python's loader."""
    exe = str(tmp_path / "sanitize_scan_model")
    csrc = os.path.join(ROOT, "slam-sam_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                        "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                        os.path.join(ROOT, "tests", "cpp", "sanitize_scan_model.cpp"), os.path.join(csrc, "ndt_scan_model.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("PASS"), r.stdout[-2000:]


# --------------------------------------------------------------------------- kernel resources
def test_unproject_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_unproject.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "u.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and name and "k_unproject" in name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    kernels = sorted(re.search(r"k_unproject_[a-z]+", n).group(0) for n in usage)
    assert kernels == ["k_unproject_aligned", "k_unproject_count", "k_unproject_emit"], sorted(usage)
    # LDS: the knot table (6144 B) and the block's columns (4096 B) where the kernel moves points, the columns alone in the
    # count pass, 16 B of wave counts in the two compaction kernels -- the figures DESIGN 7h quotes
    lds = {"k_unproject_aligned": 10240, "k_unproject_count": 4112, "k_unproject_emit": 10256}
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["LDS"] == lds[re.search(r"k_unproject_[a-z]+", name).group(0)], (name, u)


def test_the_motion_and_the_predicate_have_one_definition():
    """dsk_keep and dsk_move are defined in ndt_deskew_device.h and nowhere else: the fused kernels and the deskew's
    call the same routines"""
    csrc = os.path.join(ROOT, "slam-sam_amd", "csrc")
    for fn in ("dsk_keep", "dsk_move", "dsk_load_table"):
        sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip", ".cpp"))]
        defs = [f for f in sources if re.search(r"\bbool %s\(|\bvoid %s\(" % (fn, fn), open(os.path.join(csrc, f)).read())]
        assert defs == ["ndt_deskew_device.h"], (fn, defs)
        for f in ("ndt_deskew.hip", "ndt_unproject.hip"):
            assert re.search(r"\b%s\(" % fn, open(os.path.join(csrc, f)).read()), (fn, f)
