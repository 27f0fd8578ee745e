"""Deskew of a 131 072-point scan with 2 and 22 knots, aligned and compacting (tuning aid, not collected by pytest; no
pass / fail number is attached -- the first numbers measured are the record):

  * per call: host clock around ndt_deskew_device on device-resident arrays (every call ends in a stream synchronise),
    profiler off;
  * per kernel: a child process under `rocprofv3 --kernel-trace --stats`; achieved GB/s = 28 bytes per point (x, y, z, t
    in, x, y, z out) over the kernel time -- for the compacting mode over the sum of its three kernels, whose count pass
    reads the 16 input bytes a second time and whose emit writes only the kept half, so its figure is a rate of useful
    bytes, not of traffic;
  * beside it what a driver can do today: the NumPy deskew of tests/test_deskew_cpu.py + setInputSource, and the host
    form putKeyframeDeskewed + setInputSourceFromKeyframe (one upload);
  * the kernels' VGPR / LDS / scratch figures as the compiler reports them.

    python tools/deskew_bench.py                 everything; writes profiles/deskew.txt
    python tools/deskew_bench.py --workload      the profiled workload itself"""
import csv
import ctypes as C
import glob
import os
import re
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N, REPS, WARMUP, BYTES_PER_POINT = 131072, 300, 20, 28


def scan_and_trajectories(pkg):
    """an Ouster-shaped scan (128 x 1024 firing order, |p| up to 120 m), its per-point alpha, a 1 m / 3 deg motion"""
    S = pkg.synth
    rng = np.random.default_rng(1)
    d = rng.normal(size=(N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = (d * rng.uniform(1.0, 120.0, (N, 1))).astype(np.float32)
    pts[:, 2] *= np.float32(0.1)
    inten = rng.uniform(0.0, 255.0, N).astype(np.float32)
    alpha = ((np.arange(N) % 1024) / 1024.0).astype(np.float32)
    Tend = S.pose_matrix(10.0, 2.0, 2.0, 0.0, 0.0, 0.3)
    traj = {}
    for k in (2, 22):
        s = np.linspace(0.0, 1.0, k)
        traj[k] = (s, np.stack([Tend @ np.linalg.inv(S.pose_matrix(1.0 - u, 0.05 * (1.0 - u), 0.0, 0.0, 0.01 * (1.0 - u),
                                                                   np.deg2rad(3.0) * (1.0 - u))) for u in s]))
    # the vehicle box and a z band that together keep about half of the scan
    filt = pkg.ScanFilter.from_vehicle_box([0.0, 0.0, 0.0], [4.0, 2.0, 2.0], z_band=(-12.0, 0.0), intensity_keep_min=250.0)
    return pts, inten, alpha, traj, filt


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


def workload(lines=None, reps=REPS):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    n_dev, info = pkg.backend_info()
    if n_dev <= 0:
        raise RuntimeError("deskew_bench: no HIP device: " + info)
    pts, inten, alpha, traj, filt = scan_and_trajectories(pkg)
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    dev = Dev()
    d = [dev.upload(pts[:, a]) for a in range(3)] + [dev.upload(alpha), dev.upload(inten)]
    o = [dev.upload(np.zeros(N, np.float32)) for _ in range(4)]
    out = [] if lines is None else lines
    out.append("device: %s" % info)
    kept = 0
    for k in (2, 22):
        kt, kp = traj[k]
        for mode, f in (("aligned", None), ("compacting", filt)):
            def call():
                return ndt.deskewDevice(d[0], d[1], d[2], d[3], N, kt, kp, o[0], o[1], o[2], N, filter=f, d_intensity=d[4],
                                        o_intensity=o[3])
            kept = call()
            med, lo, p95 = timed(call, reps)
            out.append("  ndt_deskew_device %-10s %2d knots: %8.1f us per call (min %8.1f, p95 %8.1f), %6d of %d points out"
                       % (mode, k, med, lo, p95, kept, N))
    if lines is not None:   # (the driver-side comparisons are not part of the profiled workload)
        from test_deskew_cpu import deskew_numpy
        kt, kp = traj[22]
        cloud = np.column_stack([pts, inten])
        med, lo, p95 = timed(lambda: ndt.setInputSource(deskew_numpy(pkg.synth, pts, alpha, kt, kp).astype(np.float32)) or ndt.wait(),
                             10, 2)
        out.append("  today: NumPy deskew (f64, per segment) + setInputSource, 22 knots: %9.1f us per scan (min %9.1f)" % (med, lo))
        med, lo, p95 = timed(lambda: ndt.setInputSource(pts) or ndt.wait(), 50, 5)
        out.append("  ... of which setInputSource of the scan alone:                      %9.1f us per scan (min %9.1f)" % (med, lo))

        def put(f):
            ndt.putKeyframeDeskewed(1, cloud, alpha, kt, kp, filter=f, intensity_column=3)
            ndt.setInputSourceFromKeyframe(1)
        for mode, f in (("aligned", None), ("compacting", filt)):
            med, lo, p95 = timed(lambda: put(f), 50, 5)
            out.append("  putKeyframeDeskewed %-10s + setInputSourceFromKeyframe, 22 knots: %9.1f us per scan (min %9.1f)"
                       % (mode, med, lo))
    print("workload: %d points, filter keeps %d" % (N, kept))
    return out


def kernel_times(out):
    with tempfile.TemporaryDirectory() as dd:
        # a time limit of its own; on expiry the whole process group goes (rocprofv3 AND the workload under it), and
        # nothing more is started on the GPU
        child = subprocess.Popen(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", dd, "-o", "dsk", "--",
                                  sys.executable, os.path.abspath(__file__), "--workload"], stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            _, err = child.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            os.killpg(child.pid, signal.SIGKILL)
            child.communicate()
            raise SystemExit("deskew_bench: the profiled child did not finish in 240 s; stopped, nothing more is started")
        p = subprocess.CompletedProcess(child.args, child.returncode, "", err)
        if p.returncode != 0:
            out.append("rocprofv3 exited with %d: %s" % (p.returncode, p.stderr[-500:]))
            return
        t = {}
        for path in glob.glob(os.path.join(dd, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    m = re.search(r"k_deskew_[a-z]+|k_filter_scan", r["Name"])
                    if m:
                        t[m.group(0)] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3)
        for name, (calls, avg, lo, hi) in sorted(t.items()):
            out.append("  %-18s calls %5d   avg %7.2f us   min %7.2f   max %7.2f   (2 and 22 knots together)" % (name, calls, avg, lo, hi))
        gb = lambda us: N * BYTES_PER_POINT / (us * 1e-6) / 1e9   # noqa: E731
        if "k_deskew_aligned" in t:
            out.append("  aligned:    %7.2f us of kernel time per scan -> %7.1f GB/s at %d bytes per point"
                       % (t["k_deskew_aligned"][1], gb(t["k_deskew_aligned"][1]), BYTES_PER_POINT))
        if all(k in t for k in ("k_deskew_count", "k_filter_scan", "k_deskew_emit")):
            us = t["k_deskew_count"][1] + t["k_filter_scan"][1] + t["k_deskew_emit"][1]
            out.append("  compacting: %7.2f us of kernel time per scan (three kernels) -> %7.1f GB/s at %d bytes per point"
                       % (us, gb(us), BYTES_PER_POINT))


def kernel_resources(out):
    src = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_deskew.hip")
    with tempfile.TemporaryDirectory() as dd:
        p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                            "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(dd, "d.o")],
                           capture_output=True, text=True)
    name, usage = None, {}
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = re.search(r"k_deskew_[a-z]+", m.group(1))
            name = name.group(0) if name else None
        m = re.search(r"(SGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and name:
            usage.setdefault(name, []).append("%s %s" % (m.group(1).split(" [")[0], m.group(2)))
    for name in sorted(usage):
        out.append("  %-18s %s" % (name, ", ".join(usage[name])))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--workload":
        workload(None, 100)
        sys.exit(0)
    lines = ["deskew: %d points, 2 and 22 knots (tools/deskew_bench.py)" % N, "",
             "== per call, host clock around calls that end in a synchronise, profiler off (median of %d) ==" % REPS]
    workload(lines)
    lines += ["", "== kernel times (rocprofv3 --kernel-trace --stats, a run of its own) =="]
    kernel_times(lines)
    lines += ["", "== kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) =="]
    kernel_resources(lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(ROOT, "profiles", "deskew.txt"), "w") as f:
        f.write(text)
