"""Lidar packets of a 2048 x 128 frame (RNG19_RFL8_SIG16_NIR16, 16 columns per packet: 128 payloads of 24 832 bytes) with
the OS2-128's beam geometry (tests/golden/os2_128_beams.json), the bench's range gate and vehicle-box / z-band filter and a
22-knot trajectory (tuning aid, not collected by pytest; no pass / fail number is attached -- the first numbers measured
are the record).  Wall time, host clock, profiler off, of

  (a) the packet route: ndt_packet_frame_push per packet (returns without waiting: the copy to the device runs behind it),
      and ndt_keyframe_put_from_packets after the last push (pre-pass result up, decode, unprojection, compaction; awaited)
  (b) ndt_packet_columns alone over the frame's 128 payloads: the whole host pre-pass
  (c) the route without these calls: a host decode of the payloads to the range image in a plain single-threaded C++
      loop (compiled here with g++ -O2; timed and reported on its own), then ndt_keyframe_put_from_ranges

and the new kernels' VGPR / LDS / scratch figures as the compiler reports them.

    python tools/packets_bench.py [--out FILE]        writes profiles/packets.txt (or FILE)"""
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
N_COLS, N_ROWS, CPP, REPS, WARMUP = 2048, 128, 16, 200, 20

# the per-pixel host loop a driver would have to write for the range-image calls: three or four scattered reads out of a
# 12-byte record, a 5-byte write (RNG19; the column headers as ndt_packet_columns reads them)
HOST_DECODE = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
extern "C" int host_decode(const uint8_t* packets, size_t n_packets, size_t bytes, int n_cols, int n_rows, int cpp,
                           uint32_t* range_mm, uint8_t* reflectivity, float* col_t) {
  const size_t block = 12 + 12 * (size_t)n_rows;
  for (int m = 0; m < n_cols; ++m) col_t[m] = std::numeric_limits<float>::quiet_NaN();
  std::memset(range_mm, 0, sizeof(uint32_t) * (size_t)n_cols * n_rows);
  std::memset(reflectivity, 0, (size_t)n_cols * n_rows);
  double t_ref = -1.0;
  int columns = 0;
  for (size_t k = 0; k < n_packets; ++k) {
    const uint8_t* p = packets + k * bytes;
    uint16_t type;
    std::memcpy(&type, p, 2);
    if (type != 1) continue;
    for (int c = 0; c < cpp; ++c) {
      const uint8_t* b = p + 32 + (size_t)c * block;
      uint64_t ns;
      uint16_t m_id;
      std::memcpy(&ns, b, 8);
      std::memcpy(&m_id, b + 8, 2);
      if (m_id >= n_cols || !(b[10] & 1)) continue;
      const double ts = std::fmod((double)ns * 1e-9, 86400.0);
      if (t_ref < 0.0) t_ref = ts;
      col_t[m_id] = (float)std::fmax(0.0, ts - t_ref);
      uint32_t* r = range_mm + (size_t)m_id * n_rows;
      uint8_t* f = reflectivity + (size_t)m_id * n_rows;
      for (int row = 0; row < n_rows; ++row) {
        const uint8_t* px = b + 12 + 12 * (size_t)row;
        uint32_t d0;
        std::memcpy(&d0, px, 4);
        r[row] = d0 & 0x0007FFFFu;
        f[row] = px[4];
      }
      ++columns;
    }
  }
  return columns;
}
"""


def frame(pkg):
    """the model, a range image of synth's analytic scene from a moving sensor, its payloads, gate, filter, 22 knots"""
    S = pkg.synth
    with open(os.path.join(ROOT, "tests", "golden", "os2_128_beams.json")) as f:
        b = json.load(f)
    model = pkg.scan_model_from_beams(N_COLS, b["beam_azimuth_angles"], b["beam_altitude_angles"], b["lidar_origin_to_beam_origin_mm"],
                                      S.pose_matrix(0.1, 0.0, 0.3, 0.0, 0.0, 0.0))
    kt = np.linspace(0.0, 0.1, 22)
    kp = np.stack([S.pose_matrix(2.0 + 12.0 * t, -3.0 + 2.0 * t, 2.0 + 0.5 * t, 0.2 * t, -0.1 * t, 0.3 + np.deg2rad(40.0) * t) for t in kt])
    ts_ns = np.uint64(1_700_000_000 * 10 ** 9) + np.arange(N_COLS, dtype=np.uint64) * np.uint64(10 ** 8 // N_COLS)
    col_t = ((ts_ns - ts_ns[0]).astype(np.float64) * 1e-9).astype(np.float32)
    img = S.range_image(model, kt, kp, col_t, seed=1, no_return=0.05)
    rng = np.random.default_rng(2)
    signal, nir = (rng.integers(0, 2 ** 16, img["range_mm"].shape).astype(np.uint16) for _ in range(2))
    packets = S.encode_packets(N_COLS, N_ROWS, pkg.LIDAR_PROFILE_RNG19, CPP, np.minimum(img["range_mm"], 2 ** 19 - 1), img["reflectivity"],
                               signal, nir, ts_ns, frame_id=1, seed=3)
    gate = pkg.RangeGate(0.5, 120.0)
    filt = pkg.ScanFilter.from_vehicle_box([0.0, 0.0, 0.0], [4.0, 2.0, 2.0], z_band=(-12.0, 1.0), intensity_keep_min=250.0)
    return model, np.ascontiguousarray(packets), gate, filt, kt, kp


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[int(len(t) * 0.95)]


def timed(fn, reps=REPS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return stats(t)


def read_source(pkg, ndt):
    n = ndt.sourceSize()
    out = np.zeros((n, 3), np.float32)
    eye = np.eye(4, dtype=np.float32).ravel()
    assert pkg.lib().ndt_transform_source(ndt._h, eye.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)), n) == 0
    return out


def workload(out, tmp):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    n_dev, info = pkg.backend_info()
    if n_dev <= 0:
        raise RuntimeError("packets_bench: no HIP device: " + info)
    src, so = os.path.join(tmp, "host_decode.cpp"), os.path.join(tmp, "host_decode.so")
    with open(src, "w") as f:
        f.write(HOST_DECODE)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    host = C.CDLL(so)
    host.host_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    model, packets, gate, filt, kt, kp = frame(pkg)
    k, size = packets.shape
    n = N_COLS * N_ROWS
    L = pkg.lib()
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0)
    ndt.setScanModel(*model)
    ndt.setPacketFormat(pkg.LIDAR_PROFILE_RNG19, CPP)
    assert ndt.packetFormat()[2] == size
    out.append("device: %s" % info)
    out.append("frame: %d x %d = %d pixels in %d payloads of %d bytes (%d bytes up; the range image is %d bytes)"
               % (N_COLS, N_ROWS, n, k, size, k * size, 5 * n + 4 * N_COLS))
    row = "  %-62s %9.1f us (min %9.1f, p95 %9.1f)%s"

    # (a) the packet route, packet by packet as a socket delivers
    sizes = np.full(k, size, np.uintp)
    taken = C.c_size_t(0)
    push_t, put_t, frame_t, put_again_t, push_all_t, put_all_t = [], [], [], [], [], []
    kept = 0
    for rep in range(WARMUP + REPS):
        t_frame = time.perf_counter()
        ndt.beginPacketFrame()
        per = []
        for j in range(k):
            t0 = time.perf_counter()
            rc = L.ndt_packet_frame_push(ndt._h, packets.ctypes.data + j * size, sizes.ctypes.data + 8 * j, 1, size, C.byref(taken))
            per.append((time.perf_counter() - t0) * 1e6)
            assert rc == 0 and taken.value == 1
        t0 = time.perf_counter()
        kept = ndt.putKeyframeFromPackets(1, kt, kp, gate=gate, filter=filt)
        t1 = time.perf_counter()
        # ... and once more with every payload long on the device, as when the packets arrive spread over the frame's 100 ms
        ndt.putKeyframeFromPackets(1, kt, kp, gate=gate, filter=filt)
        t2 = time.perf_counter()
        # the whole frame in ONE push (one copy), then the put
        ndt.beginPacketFrame()
        t3 = time.perf_counter()
        rc = L.ndt_packet_frame_push(ndt._h, packets.ctypes.data, sizes.ctypes.data, k, size, C.byref(taken))
        t4 = time.perf_counter()
        assert rc == 0 and taken.value == k
        ndt.putKeyframeFromPackets(1, kt, kp, gate=gate, filter=filt)
        t5 = time.perf_counter()
        if rep >= WARMUP:
            push_t += per
            put_t.append((t1 - t0) * 1e6)
            frame_t.append((t1 - t_frame) * 1e6)
            put_again_t.append((t2 - t1) * 1e6)
            push_all_t.append((t4 - t3) * 1e6)
            put_all_t.append((t5 - t4) * 1e6)
    ndt.setInputSourceFromKeyframe(1)
    from_packets = read_source(pkg, ndt)
    out.append("(a) the packet route, %d points kept by gate and filter" % kept)
    out.append(row % ("ndt_packet_frame_push, one payload per call", *stats(push_t), " per packet"))
    out.append(row % ("ndt_keyframe_put_from_packets after the last push", *stats(put_t), " per frame"))
    out.append(row % ("begin + %d pushes back to back + put, end to end" % k, *stats(frame_t), " per frame"))
    out.append(row % ("ndt_keyframe_put_from_packets, every payload long on the device", *stats(put_again_t), " per frame"))
    out.append("  %-62s %9.1f us per frame (%d x the push median + that put's median)"
               % ("host time of a frame whose packets arrive spread out", k * stats(push_t)[0] + stats(put_again_t)[0], k))
    out.append(row % ("ndt_packet_frame_push, all %d payloads in one call" % k, *stats(push_all_t), " per frame"))
    out.append(row % ("  then ndt_keyframe_put_from_packets", *stats(put_all_t), " per frame"))

    # (b) the host pre-pass alone
    col_src, col_t = np.zeros(N_COLS, np.int32), np.zeros(N_COLS, np.float32)
    info_s = pkg.PacketFrameInfo()
    med_b = timed(lambda: L.ndt_packet_columns(pkg.LIDAR_PROFILE_RNG19, CPP, N_COLS, N_ROWS, packets.ctypes.data, sizes.ctypes.data, k, size,
                                               float("nan"), col_src.ctypes.data, col_t.ctypes.data, C.byref(info_s)))
    out.append("(b) the host pre-pass")
    out.append(row % ("ndt_packet_columns over the %d payloads (%d column headers)" % (k, N_COLS), *med_b, " per frame"))

    # (c) the route the range-image calls offer: a per-pixel host decode, then ndt_keyframe_put_from_ranges
    r, refl, t = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(N_COLS, np.float32)
    decode = lambda: host.host_decode(packets.ctypes.data, k, size, N_COLS, N_ROWS, CPP, r.ctypes.data, refl.ctypes.data, t.ctypes.data)   # noqa: E731
    assert decode() == N_COLS
    med_h = timed(decode)
    med_p = timed(lambda: ndt.putKeyframeFromRanges(2, r, refl, t, kt, kp, gate=gate, filter=filt))
    out.append("(c) the route without the packet calls")
    out.append(row % ("host decode to the range image, single-threaded C++ (g++ -O2)", *med_h, " per frame"))
    out.append(row % ("  then ndt_keyframe_put_from_ranges", *med_p, " per frame"))
    out.append("  %-62s %9.1f us per frame (sum of the two medians)" % ("that route in all", med_h[0] + med_p[0]))
    ndt.setInputSourceFromKeyframe(2)
    from_ranges = read_source(pkg, ndt)
    same = from_ranges.shape == from_packets.shape and from_ranges.tobytes() == from_packets.tobytes()
    out.append("the two archive entries: %d and %d points, %s" % (len(from_packets), len(from_ranges), "bit for bit equal" if same else "DIFFERENT"))
    ndt.close()


def kernel_resources(out):
    src = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_packets.hip")
    with tempfile.TemporaryDirectory() as dd:
        p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                            "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(dd, "p.o")],
                           capture_output=True, text=True)
    name, usage = None, {}
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = re.search(r"k_decode_packets|k_gather_u16", m.group(1))
            name = name.group(0) if name else None
        m = re.search(r"(SGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and name:
            usage.setdefault(name, []).append("%s %s" % (m.group(1).split(" [")[0], m.group(2)))
    for name in sorted(usage):
        out.append("  %-20s %s" % (name, ", ".join(usage[name])))


if __name__ == "__main__":
    path = os.path.join(ROOT, "profiles", "packets.txt")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    lines = ["packets: a %d x %d frame as %d-column RNG19 payloads, OS2-128 beam geometry (tools/packets_bench.py)" % (N_COLS, N_ROWS, CPP), "",
             "== wall time, host clock, profiler off (medians of %d frames; the push of %d x as many calls) ==" % (REPS, N_COLS // CPP)]
    with tempfile.TemporaryDirectory() as tmp:
        workload(lines, tmp)
    lines += ["", "== kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) =="]
    kernel_resources(lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(path, "w") as f:
        f.write(text)
