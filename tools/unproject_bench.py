"""Unprojection of a 2048 x 128 range image with the OS2-128's beam geometry (tests/golden/os2_128_beams.json), the range
gate, the vehicle-box / z-band filter and a 22-knot trajectory (tuning aid, not collected by pytest; no pass / fail number
is attached -- the first numbers measured are the record).  Wall time, host clock around calls that end in a stream
synchronise, profiler off, of

  * ndt_keyframe_put_from_ranges             the range image as received -> the archive entry (one 5-byte-per-pixel upload)
  * ndt_unproject                            the host form: the same upload, the compacted cloud back on the host
  * ndt_unproject_device                     device-resident range image and outputs: the launches alone
  * the route without these calls to the same archive entry: the unprojection, the gate, the filter and the compaction in
    NumPy on the host (timed and reported on its own), then ndt_keyframe_put_deskewed of the points, times and
    intensities it leaves

and the kernels' VGPR / LDS / scratch figures as the compiler reports them.

    python tools/unproject_bench.py [--out FILE]        writes profiles/unproject.txt (or FILE)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_COLS, N_ROWS, REPS, WARMUP = 2048, 128, 200, 20


def frame(pkg):
    """the model, a range image of synth's analytic scene from a sensor moving 1.2 m / 4 degrees, gate, filter, 22 knots"""
    S = pkg.synth
    with open(os.path.join(ROOT, "tests", "golden", "os2_128_beams.json")) as f:
        b = json.load(f)
    model = pkg.scan_model_from_beams(N_COLS, b["beam_azimuth_angles"], b["beam_altitude_angles"], b["lidar_origin_to_beam_origin_mm"],
                                      S.pose_matrix(0.1, 0.0, 0.3, 0.0, 0.0, 0.0))
    kt = np.linspace(0.0, 0.1, 22)
    kp = np.stack([S.pose_matrix(2.0 + 12.0 * t, -3.0 + 2.0 * t, 2.0 + 0.5 * t, 0.2 * t, -0.1 * t, 0.3 + np.deg2rad(40.0) * t) for t in kt])
    col_t = np.linspace(0.0, 0.1, N_COLS, endpoint=False).astype(np.float32)
    img = S.range_image(model, kt, kp, col_t, seed=1, no_return=0.05)
    gate = pkg.RangeGate(0.5, 120.0)
    filt = pkg.ScanFilter.from_vehicle_box([0.0, 0.0, 0.0], [4.0, 2.0, 2.0], z_band=(-12.0, 1.0), intensity_keep_min=250.0)
    return model, img, gate, filt, kt, kp


def host_unprojection(model, img, gate, filt):
    """what the lidar callback does per pixel, vectorised in float32: the points it would push, their times and
    reflectivities, in pixel order"""
    x1, y1, z1, x2, y2, z2 = model
    r, refl, t = img["range_mm"], img["reflectivity"], img["col_t"]
    rm = r.astype(np.float32) * np.float32(0.001)
    x, y, z = rm * x1 + x2[:, None], rm * y1 + y2[:, None], rm * z1 + z2[:, None]
    keep = (r != 0) & np.isfinite(t)[:, None] & (np.float32(gate.range_min) <= rm) & (rm <= np.float32(gate.range_max))
    lo, hi = np.array(filt.box_min[:], np.float32), np.array(filt.box_max[:], np.float32)
    keep &= ~((lo[0] <= x) & (x <= hi[0]) & (lo[1] <= y) & (y <= hi[1]) & (lo[2] <= z) & (z <= hi[2]))
    keep &= ((np.float32(filt.z_min) <= z) & (z <= np.float32(filt.z_max))) | (refl >= np.float32(filt.intensity_keep_min))
    cloud = np.stack([x[keep], y[keep], z[keep], refl[keep].astype(np.float32)], 1)
    return np.ascontiguousarray(cloud), np.ascontiguousarray(np.broadcast_to(t[:, None], r.shape)[keep])


class Dev:
    def __init__(self):
        self.rt = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        self.rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), max(a.nbytes, 4)) == 0
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p.value


def timed(fn, reps=REPS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    t.sort()
    return t[len(t) // 2], t[0], t[int(len(t) * 0.95)]


def read_source(pkg, ndt):
    n = ndt.sourceSize()
    out = np.zeros((n, 3), np.float32)
    eye = np.eye(4, dtype=np.float32).ravel()
    assert pkg.lib().ndt_transform_source(ndt._h, eye.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)), n) == 0
    return out


def workload(out):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    n_dev, info = pkg.backend_info()
    if n_dev <= 0:
        raise RuntimeError("unproject_bench: no HIP device: " + info)
    model, img, gate, filt, kt, kp = frame(pkg)
    r, refl, t = img["range_mm"], img["reflectivity"], img["col_t"]
    n = r.size
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    ndt.setScanModel(*model)
    out.append("device: %s" % info)
    row = "  %-58s %9.1f us per frame (min %9.1f, p95 %9.1f)%s"

    kept = ndt.putKeyframeFromRanges(1, r, refl, t, kt, kp, gate=gate, filter=filt)
    out.append("frame: %d x %d = %d pixels, %d with a return, %d kept by gate and filter; 22 knots" % (N_COLS, N_ROWS, n, int((r != 0).sum()), kept))
    out.append("bytes per frame: %d in (4 + 1 per pixel, 4 per column), tables %d resident (read per frame: 12 per pixel + 12 per "
               "column), %d out (12 per kept point into the archive)" % (5 * n + 4 * N_COLS, 12 * n + 12 * N_COLS, 12 * kept))
    ndt.setInputSourceFromKeyframe(1)
    fused = read_source(pkg, ndt)
    med, lo, p95 = timed(lambda: ndt.putKeyframeFromRanges(1, r, refl, t, kt, kp, gate=gate, filter=filt))
    out.append(row % ("ndt_keyframe_put_from_ranges (gate, filter, 22 knots)", med, lo, p95, ""))
    med, lo, p95 = timed(lambda: ndt.unproject(r, refl, t, kt, kp, gate=gate, filter=filt))
    out.append(row % ("ndt_unproject, host form, compacting", med, lo, p95, ""))
    med, lo, p95 = timed(lambda: ndt.unproject(r, refl, t, kt, kp, gate=gate), 50, 5)
    out.append(row % ("ndt_unproject, host form, organised (all %d points back)" % n, med, lo, p95, ""))
    dev = Dev()
    d_r, d_refl, d_t = dev.upload(r), dev.upload(refl), dev.upload(t)
    o = [dev.upload(np.zeros(n, np.float32)) for _ in range(5)]
    for mode, f in (("organised", None), ("compacting", filt)):
        def call():
            return ndt.unprojectDevice(d_r, d_refl, d_t, o[0], o[1], o[2], n, knot_t=kt, knot_poses=kp, gate=gate, filter=f,
                                       o_intensity=o[3], o_t=o[4])
        m = call()
        med, lo, p95 = timed(call)
        out.append(row % ("ndt_unproject_device %s" % mode, med, lo, p95, ", %d points out" % m))
    # the route without these calls: the host forms the points, the deskew call archives them
    cloud, tt = host_unprojection(model, img, gate, filt)
    med_h, lo_h, p95_h = timed(lambda: host_unprojection(model, img, gate, filt), 20, 3)
    out.append(row % ("host unprojection + gate + filter + compaction in NumPy (f32)", med_h, lo_h, p95_h, ", %d points" % len(cloud)))
    med_p, lo_p, p95_p = timed(lambda: ndt.putKeyframeDeskewed(2, cloud, tt, kt, kp, intensity_column=3))
    out.append(row % ("  then ndt_keyframe_put_deskewed of those points", med_p, lo_p, p95_p, ""))
    out.append("  %-58s %9.1f us per frame (sum of the two medians)" % ("that route in all", med_h + med_p))
    ndt.setInputSourceFromKeyframe(2)
    composed = read_source(pkg, ndt)
    if composed.shape == fused.shape:
        out.append("the two archive entries: %d points each, largest difference %.3e m (NumPy rounds the product and the sum, "
                   "the kernel fuses them)" % (len(fused), float(np.abs(composed - fused).max()) if len(fused) else 0.0))
    else:
        out.append("the two archive entries differ in size: %d fused, %d composed (a point on a filter bound)" % (len(fused), len(composed)))
    ndt.close()


def kernel_resources(out):
    src = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_unproject.hip")
    with tempfile.TemporaryDirectory() as dd:
        p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                            "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(dd, "u.o")],
                           capture_output=True, text=True)
    name, usage = None, {}
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = re.search(r"k_unproject_[a-z]+", m.group(1))
            name = name.group(0) if name else None
        m = re.search(r"(SGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and name:
            usage.setdefault(name, []).append("%s %s" % (m.group(1).split(" [")[0], m.group(2)))
    for name in sorted(usage):
        out.append("  %-20s %s" % (name, ", ".join(usage[name])))


if __name__ == "__main__":
    path = os.path.join(ROOT, "profiles", "unproject.txt")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    lines = ["unproject: a %d x %d range image, OS2-128 beam geometry (tools/unproject_bench.py)" % (N_COLS, N_ROWS), "",
             "== per call, host clock around calls that end in a synchronise, profiler off (median of %d) ==" % REPS]
    workload(lines)
    lines += ["", "== kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) =="]
    kernel_resources(lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(path, "w") as f:
        f.write(text)
