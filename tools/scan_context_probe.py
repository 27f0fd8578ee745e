"""Scan Context on the device: time per descriptor and per match (tuning aid, not collected by pytest).

    python tools/scan_context_probe.py [--out FILE] [--small]

Default parameters (20 rings x 60 sectors, 80 m).  Every call is complete when it returns, so a host clock around it measures
launches, kernels, read-back and the wait; warmed up, many repetitions, median and the 10 % / 90 % points.  Reported:
  - ndt_scan_context_device for a 65 536-point and a 131 072-point device-resident scan (points of a ring pattern within
    95 m, a sixth of them beyond the radius gate); beside each the floor of one plain read of the scan, 3 * 4 * n bytes at
    the copy bandwidth measured in the same process (a 256 MiB device-to-device hipMemcpy: bytes read + bytes written over
    its time);
  - ndt_scan_context_match (query from the host) and ndt_scan_context_match_keyframe (query in the bank) against banks of
    1 000, 10 000 and 100 000 entries; beside each the f64 work of the rule, S * S * R multiply-add pairs per entry, at the
    device's vector f64 rate (78.6 TFLOP/s by its public specification, 2 FLOP per pair);
  - the same two operations in the NumPy restatement of tests/test_scan_context_cpu.py on the host, for scale.
No pass / fail number is attached.  Writes what it prints to profiles/scan_context.txt (or --out)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

F64_RATE = 78.6e12
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    ts = np.array(ts)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def scan_like(n, seed):
    """a lidar-like cloud: 128 elevation rings, ranges spread to 95 m, float32 [n, 3]"""
    rng = np.random.default_rng(seed)
    az = rng.uniform(0.0, 2 * np.pi, n)
    r = 95.0 * rng.random(n) ** 0.7
    el = np.deg2rad(rng.integers(0, 128, n) * (45.0 / 127.0) - 22.5)
    return np.stack([r * np.cos(az), r * np.sin(az), r * np.tan(el)], 1).astype(np.float32)


def main():
    out = os.path.join(ROOT, "profiles", "scan_context.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    small = "--small" in sys.argv
    pkg = ge.load_package()
    from test_scan_context_cpu import scan_context_match_numpy, scan_context_numpy
    n_dev, info = pkg.backend_info()
    if n_dev <= 0:
        raise RuntimeError("scan_context_probe: no HIP device: " + info)
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    prm = pkg.getScanContextParams(ndt)
    R, S = prm["n_rings"], prm["n_sectors"]
    dirs = pkg.scanContextSectorTable(S)
    rt = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipFree.argtypes = [C.c_void_p]

    def dev_alloc(nbytes):
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), nbytes) == 0
        return p.value

    def upload(a):
        a = np.ascontiguousarray(a)
        p = dev_alloc(max(a.nbytes, 4))
        assert rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    say("Scan Context on the device (DESIGN 7m) -- tools/scan_context_probe.py; %s" % info)
    say("parameters: %d rings x %d sectors, %.0f m; every call awaited, host clock, median (10 %%, 90 %%)" % (R, S, prm["max_radius"]))

    # the copy bandwidth of this process: a large device-to-device hipMemcpy, awaited
    nbytes = (32 if small else 256) << 20
    a, b = dev_alloc(nbytes), dev_alloc(nbytes)

    def copy():
        assert rt.hipMemcpy(b, a, nbytes, 3) == 0
        assert rt.hipDeviceSynchronize() == 0

    t = timed(copy, 20, warm=3)
    bw = 2.0 * nbytes / t[0]
    say("copy bandwidth: %.2f TB/s (hipMemcpy device to device, %d MiB, read + written bytes over %.3f ms)" % (bw / 1e12, nbytes >> 20, 1e3 * t[0]))
    rt.hipFree(a)
    rt.hipFree(b)

    d_desc, d_count = dev_alloc(4 * R * S), dev_alloc(4 * R * S)
    host = {}
    for n in ((4096, 8192) if small else (65536, 131072)):
        cloud = scan_like(n, seed=n)
        soa = [upload(cloud[:, k]) for k in range(3)]
        t = timed(lambda: pkg.scanContextDevice(ndt, soa[0], soa[1], soa[2], n, d_desc, d_count), 500, warm=20)
        floor = 12.0 * n / bw
        say("ndt_scan_context_device, %6d points: %7.1f us (%.1f, %.1f); one read of the scan at the copy bandwidth: %.2f us"
            % (n, 1e6 * t[0], 1e6 * t[1], 1e6 * t[2], 1e6 * floor))
        host[n] = cloud
        for p in soa:
            rt.hipFree(p)

    rng = np.random.default_rng(5)
    pool = [(rng.uniform(0.0, 12.0, (R, S)) * (rng.random((R, S)) < 0.35)).astype(np.float32) for _ in range(64)]
    query = pool[7] + (rng.random((R, S)) < 0.05).astype(np.float32)
    have = 0
    for m in ((100, 1000) if small else (1000, 10000, 100000)):
        for i in range(have, m):
            pkg.scanContextBankPut(ndt, i, pool[i % 64])
        have = m
        pairs = float(S) * S * R * m
        for name, fn in (("ndt_scan_context_match", lambda: pkg.scanContextMatch(ndt, query)),
                         ("ndt_scan_context_match_keyframe", lambda: pkg.scanContextMatchKeyframe(ndt, 7))):
            t = timed(fn, 100 if m <= 10000 else 30, warm=5)
            say("%-32s %6d entries: %9.1f us (%.1f, %.1f), %.3f us per entry; %.3g multiply-add pairs at %.1f TFLOP/s f64: %.1f us"
                % (name + ",", m, 1e6 * t[0], 1e6 * t[1], 1e6 * t[2], 1e6 * t[0] / m, pairs, F64_RATE / 1e12, 1e6 * 2.0 * pairs / F64_RATE))

    # the NumPy restatement on the host, for scale (once each: seconds, not microseconds)
    n = min(host)
    t0 = time.perf_counter()
    scan_context_numpy(host[n], dirs, **prm)
    t1 = time.perf_counter()
    bank = np.stack([pool[i % 64] for i in range(100 if small else 1000)])
    scan_context_match_numpy(query, bank)
    t2 = time.perf_counter()
    say("NumPy restatement on the host: descriptor of %d points %.1f ms; match against %d entries %.1f ms (%.1f us per entry)"
        % (n, 1e3 * (t1 - t0), len(bank), 1e3 * (t2 - t1), 1e6 * (t2 - t1) / len(bank)))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
