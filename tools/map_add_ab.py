"""Two library builds against each other on ONE box, for the voxel map's calls (tuning aid, not collected by pytest): what
tools/lib_ab.py does for the align step -- child processes that alternate between the libraries (A B A B ...), so
box-to-box differences and drift cancel -- for ndt_map_add_device, ndt_map_export_device, ndt_set_target_from_map and, on
a second handle whose resolution is the map's leaf, ndt_set_target_from_map_moments (100 m box around the last pose).

    python tools/map_add_ab.py <libA.so> <libB.so> [rounds]     (names relative to slam-sam_amd/)

A child talks to its library through ctypes on the C-ABI directly (not through the package's binding, which binds every
symbol of the current header), so a library of an earlier commit can stand on one side.  65 536-point scans of the
synthetic street, leaf 0.5 m, median of 15 per step (as tools/voxel_map_bench.py).  The spread between the rounds of one
library is the tool's own run-to-run margin."""
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEAF, REPS = 0.5, 15


def child(path, tag):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()                                   # Params, the synthetic street, the HIP helper: no library call
    from slam_sam_amd import replay
    L = C.CDLL(path)
    vp = C.c_void_p
    L.ndt_default_params.argtypes = [C.POINTER(pkg.Params)]
    L.ndt_create.argtypes = [C.POINTER(pkg.Params), C.POINTER(vp)]
    L.ndt_destroy.argtypes = [vp]
    L.ndt_map_reset.argtypes = [vp, C.c_float, C.c_int, C.c_int64]
    L.ndt_map_add_device.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_double)]
    L.ndt_map_export_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ndt_set_target_from_map.argtypes = [vp, C.c_int]
    L.ndt_wait.argtypes = [vp]
    L.ndt_map_enable_moments.argtypes = [vp]
    L.ndt_set_target_from_map_moments.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    prm = pkg.Params()
    L.ndt_default_params(C.byref(prm))
    prm.resolution, prm.device_id = 1.0, 0
    h = vp()
    assert L.ndt_create(C.byref(prm), C.byref(h)) == 0
    hip = pkg.ranks.Hip(0)
    stream = replay.make_stream(n_frames=16, beams=128, cols=512)
    scans = [pkg.synth.transform(T, s).astype(np.float32) for s, T in stream]
    n = len(scans[0])
    d = [[hip.upload(np.ascontiguousarray(s[:, a])) for a in range(3)] for s in scans]
    o = [hip.upload(np.zeros(16 * n, np.float32)) for _ in range(3)]

    def ok(rc):
        assert rc == 0, rc

    def med(fn, before=None):
        ts = []
        for _ in range(REPS):
            if before:
                before()
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        return 1e3 * float(np.median(ts))

    def add(k):
        ok(L.ndt_map_add_device(h, d[k][0], d[k][1], d[k][2], None, n, None))

    def reset():
        ok(L.ndt_map_reset(h, LEAF, 0, 0))

    def export():
        m = C.c_size_t(0)
        ok(L.ndt_map_export_device(h, 1, o[0], o[1], o[2], None, None, 16 * n, C.byref(m)))

    def target():
        ok(L.ndt_set_target_from_map(h, 1))
        ok(L.ndt_wait(h))

    reset()
    for _ in range(3):
        add(0)
    t0 = med(lambda: add(0), before=reset)
    reset()
    for k in range(16):
        add(k)
    t1 = med(lambda: add(1))
    export()
    t2 = med(export)
    target()
    t3 = med(target)
    # the target from the moments of the same 16 scans
    prm.resolution = LEAF
    h2 = vp()
    assert L.ndt_create(C.byref(prm), C.byref(h2)) == 0
    ok(L.ndt_map_reset(h2, LEAF, 0, 0))
    ok(L.ndt_map_enable_moments(h2))
    for k in range(16):
        ok(L.ndt_map_add_device(h2, d[k][0], d[k][1], d[k][2], None, n, None))
    c = stream[15][1][:3, 3]
    lo, hi = (C.c_float * 3)(*(c - 50.0)), (C.c_float * 3)(*(c + 50.0))

    def moments_target():
        ok(L.ndt_set_target_from_map_moments(h2, lo, hi))

    moments_target()
    t4 = med(moments_target)
    print("%-34s add into an empty map %7.3f ms | into the 16-scan map %7.3f ms | export %7.3f ms | setInputTargetFromMap %7.3f ms"
          " | setInputTargetFromMapMoments %7.3f ms" % (tag, t0, t1, t2, t3, t4), flush=True)
    L.ndt_destroy(h2)
    L.ndt_destroy(h)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], args[2])
    rounds = int(args.pop()) if args and args[-1].isdigit() else 3
    for r in range(rounds):
        for lib in args:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.join(ROOT, "slam-sam_amd", lib),
                                "%s #%d" % (lib, r)], capture_output=True, text=True, timeout=300)
            out = [ln for ln in p.stdout.splitlines() if " ms" in ln]
            print(out[-1] if out else "FAILED %s: %s" % (lib, p.stderr[-400:]), flush=True)
            if not out:
                return 1          # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
