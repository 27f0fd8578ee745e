"""Lidar packets on the host: ndt_packet_columns against a NumPy restatement of the format table of include/ndt_hip.h
(packet and column rules, the fmod / max / float32 time rule), an arrival-order restatement of the reference's decoder
against NumPy decode + the existing NumPy unprojection, that host code under AddressSanitizer + UBSan as a stand-alone
program, and the new kernels' resource use.  No GPU.  The helpers are shared with tests/test_gpu_packets.py."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_deskew import bits, keep_numpy
from test_gpu_unproject import fma_f32, organised_numpy, random_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RNG19, LEGACY = 0, 1
INVALID_ARG = -1
COUNTERS = ("frame_id", "next_frame_pending", "n_columns", "n_packets", "n_packets_accepted", "n_packets_bad_size",
            "n_packets_bad_type", "n_columns_bad_id", "n_columns_bad_frame", "n_columns_bad_status", "n_columns_overridden")
DAY_NS = 86400 * 10 ** 9


# --------------------------------------------------------------------------- the restatement
def layout(profile, cpp, n_rows):
    """(packet header, block, first pixel in a block, packet bytes, slot bytes): the table of include/ndt_hip.h"""
    legacy = profile == LEGACY
    first = 16 if legacy else 12
    block = first + 12 * n_rows + (4 if legacy else 0)
    size = (0 if legacy else 64) + cpp * block
    return (0 if legacy else 32), block, first, size, (size + 15) // 16 * 16


def column_ts(ts_ns):
    """fmod((double)timestamp_ns * 1e-9, 86400.0)"""
    return float(np.fmod(np.float64(np.uint64(ts_ns)) * np.float64(1e-9), np.float64(86400.0)))


def columns_numpy(profile, cpp, n_cols, n_rows, packets, t_ref=None):
    """The host pre-pass restated: packets is a sequence of bytes-like payloads in arrival order.  Returns (col_src int32,
    col_t float32, info dict, packed: the accepted packets in arrival order, each padded to its 16-byte-aligned slot, as a
    uint32 array -- what col_src indexes)."""
    header, block, first, size, slot = layout(profile, cpp, n_rows)
    legacy = profile == LEGACY
    info = dict.fromkeys(COUNTERS, 0)
    info["frame_id"] = -1
    src, ts = np.full(n_cols, -1, np.int32), np.zeros(n_cols, np.float64)
    accepted, order = [], []                                  # order: ts of the accepted columns as they arrive
    capacity = 2 * ((n_cols + cpp - 1) // cpp)
    for p in packets:
        p = bytes(p)
        if len(accepted) == capacity:
            break
        if len(p) != size:
            info["n_packets"] += 1
            info["n_packets_bad_size"] += 1
            continue
        if not legacy and struct.unpack_from("<H", p, 0)[0] != 1:
            info["n_packets"] += 1
            info["n_packets_bad_type"] += 1
            continue
        frame = struct.unpack_from("<H", p, 10 if legacy else 2)[0]
        if info["frame_id"] >= 0 and frame != info["frame_id"]:
            info["next_frame_pending"] = 1
            break
        info["frame_id"] = frame
        info["n_packets"] += 1
        info["n_packets_accepted"] += 1
        k = len(accepted)
        accepted.append(p + bytes(slot - size))
        for c in range(cpp):
            b = header + c * block
            m_id = struct.unpack_from("<H", p, b + 8)[0]
            if m_id >= n_cols:
                info["n_columns_bad_id"] += 1
                continue
            if legacy:
                if struct.unpack_from("<H", p, b + 10)[0] != frame:
                    info["n_columns_bad_frame"] += 1
                    continue
                if struct.unpack_from("<I", p, b + 16 + 12 * n_rows)[0] != 0xFFFFFFFF:
                    info["n_columns_bad_status"] += 1
                    continue
            elif not p[b + 10] & 1:
                info["n_columns_bad_status"] += 1
                continue
            t = column_ts(struct.unpack_from("<Q", p, b)[0])
            order.append(t)
            info["n_columns_overridden" if src[m_id] >= 0 else "n_columns"] += 1
            src[m_id] = (k * slot + b + first) // 4
            ts[m_id] = t
    ref = float(t_ref) if t_ref is not None else (order[0] if order else np.nan)
    col_t = np.full(n_cols, np.nan, np.float32)
    live = src >= 0
    col_t[live] = np.maximum(0.0, ts[live] - ref).astype(np.float32)          # one rounding: float64 difference -> float32
    info.update(t_ref=ref, ts_first=order[0] if order else np.nan, ts_last=order[-1] if order else np.nan)
    packed = np.frombuffer(b"".join(accepted), "<u4") if accepted else np.zeros(0, np.uint32)
    return src, col_t, info, packed


def decode_numpy(profile, cpp, n_cols, n_rows, packets, t_ref=None):
    """NumPy decode of the payloads: dict(range_mm uint32, reflectivity uint8, signal, nir uint16 [n_cols, n_rows], col_t
    float32 [n_cols], info)"""
    src, col_t, info, packed = columns_numpy(profile, cpp, n_cols, n_rows, packets, t_ref)
    d = np.zeros((n_cols, n_rows, 3), np.uint32)
    for m in np.flatnonzero(src >= 0):
        d[m] = packed[src[m]:src[m] + 3 * n_rows].reshape(n_rows, 3)
    mask = np.uint32(0x000FFFFF if profile == LEGACY else 0x0007FFFF)
    return dict(range_mm=d[:, :, 0] & mask, reflectivity=(d[:, :, 1] & np.uint32(0xFF)).astype(np.uint8),
                signal=(d[:, :, 1] >> np.uint32(16)).astype(np.uint16), nir=(d[:, :, 2] & np.uint32(0xFFFF)).astype(np.uint16),
                col_t=col_t, info=info, col_src=src)


def random_frame(profile, n_cols, n_rows, seed, t0_ns=1_700_000_000 * 10 ** 9 + 123_456_789, zero_share=0.15, dt_ns=48_828):
    """a seeded range image over the profile's whole range width, with signal and nir, and column timestamps dt_ns apart
    (48 828 ns: a 2048-column frame in 100 ms) from t0_ns"""
    rng = np.random.default_rng(seed)
    top = 2 ** 20 if profile == LEGACY else 2 ** 19
    r = rng.integers(1, top, (n_cols, n_rows)).astype(np.uint32)
    r[rng.uniform(size=r.shape) < zero_share] = 0
    r.ravel()[rng.permutation(r.size)[:2]] = [top - 1, 1][:min(r.size, 2)]
    refl = rng.integers(0, 256, (n_cols, n_rows)).astype(np.uint8)
    sig = rng.integers(0, 2 ** 16, (n_cols, n_rows)).astype(np.uint16)
    nir = rng.integers(0, 2 ** 16, (n_cols, n_rows)).astype(np.uint16)
    ts = (np.uint64(t0_ns) + np.arange(n_cols, dtype=np.uint64) * np.uint64(dt_ns)).astype(np.uint64)
    return dict(range_mm=r, reflectivity=refl, signal=sig, nir=nir, ts_ns=ts)


def encode(S, profile, n_cols, n_rows, cpp, frame, frame_id=7, **kw):
    return S.encode_packets(n_cols, n_rows, profile, cpp, frame["range_mm"], frame["reflectivity"], frame["signal"], frame["nir"],
                            frame["ts_ns"], frame_id, **kw)


def disturbances(profile, n_cols, cpp):
    """name -> knobs of synth.encode_packets, every disturbance the format knows"""
    k = (n_cols + cpp - 1) // cpp
    d = {"in order": {}, "reversed": dict(order=list(range(k))[::-1]), "invalid status": dict(invalid_status=(0, n_cols - 1)),
         "bad m_id": dict(bad_m_id=(n_cols // 2,)), "duplicated": dict(duplicate=(0,))}
    if k > 1:
        d["one dropped"] = dict(order=[i for i in range(k) if i != k // 2])
        d["shuffled, dropped, duplicated"] = dict(order=list(np.random.default_rng(k).permutation(k)[:-1]), duplicate=(k - 1, 0),
                                                  invalid_status=(1,))
    if profile == LEGACY:
        d["other frame id in a column"] = dict(other_frame=(n_cols - 1,))
    elif k > 1:
        d["wrong type"] = dict(wrong_type=(1,))
    return d


def assert_same_pass(pkg, profile, cpp, n_cols, n_rows, packets, t_ref=None):
    src, col_t, info = pkg.packet_columns(profile, cpp, n_cols, n_rows, packets, t_ref)
    w_src, w_t, w_info, _ = columns_numpy(profile, cpp, n_cols, n_rows, list(packets), t_ref)
    assert np.array_equal(src, w_src)
    assert np.array_equal(bits(col_t), bits(w_t))
    for key in COUNTERS:
        assert info[key] == w_info[key], (key, info[key], w_info[key])
    for key in ("t_ref", "ts_first", "ts_last"):
        assert struct.pack("<d", info[key]) == struct.pack("<d", w_info[key]) or (np.isnan(info[key]) and np.isnan(w_info[key])), key
    return src, col_t, info


# --------------------------------------------------------------------------- 1. ndt_packet_columns
@pytest.mark.parametrize("profile", [RNG19, LEGACY])
@pytest.mark.parametrize("n_cols,n_rows,cpp", [(2, 3, 2), (24, 5, 4), (300, 1, 4), (32, 128, 16), (10, 4, 4)])
def test_packet_columns_match_the_restatement(pkg, S, profile, n_cols, n_rows, cpp):
    frame = random_frame(profile, n_cols, n_rows, 3 + n_cols)
    k = (n_cols + cpp - 1) // cpp
    for name, knobs in disturbances(profile, n_cols, cpp).items():
        packets = encode(S, profile, n_cols, n_rows, cpp, frame, seed=11, **knobs)
        assert packets.shape[1] == layout(profile, cpp, n_rows)[3]
        for t_ref in (column_ts(frame["ts_ns"][0]) - 0.25, column_ts(frame["ts_ns"][n_cols // 2]), None):   # (the checks below: automatic)
            src, col_t, info = assert_same_pass(pkg, profile, cpp, n_cols, n_rows, packets, t_ref)
        if name == "in order":
            assert info["n_columns"] == n_cols and (src >= 0).all() and col_t[0] == 0.0 and info["n_packets_accepted"] == k
            assert info["n_columns_bad_id"] == k * cpp - n_cols          # the last packet's surplus columns
        if name == "reversed" and k > 1:
            assert info["ts_first"] > info["ts_last"] and (col_t[:-cpp] == 0.0).all()   # every earlier column clamps to 0
        if name == "one dropped":
            assert info["n_columns"] == n_cols - cpp and np.isnan(col_t).sum() == cpp and (src < 0).sum() == cpp
        if name == "duplicated":
            assert info["n_columns_overridden"] == min(cpp, n_cols) and info["n_packets_accepted"] == k + 1
            assert src[0] // (layout(profile, cpp, n_rows)[4] // 4) == k   # the later arrival holds column 0
        if name == "invalid status":
            assert info["n_columns_bad_status"] == 2 and src[0] < 0 and src[n_cols - 1] < 0 and np.isnan(col_t[0])
        if name == "bad m_id":
            assert src[n_cols // 2] < 0 and info["n_columns_bad_id"] == 1 + k * cpp - n_cols
        if name == "wrong type":
            assert info["n_packets_bad_type"] == 1 and info["n_packets"] == k and info["n_packets_accepted"] == k - 1
        if name == "other frame id in a column":
            assert info["n_columns_bad_frame"] == 1 and src[n_cols - 1] < 0
    # wrong sizes among right ones: a sequence of payloads of their own lengths
    packets = [bytes(p) for p in encode(S, profile, n_cols, n_rows, cpp, frame, seed=12)]
    mixed = [packets[0][:-4]] + packets[:1] + [packets[0] + bytes(4), b""] + packets[1:]
    src, col_t, info = assert_same_pass(pkg, profile, cpp, n_cols, n_rows, mixed)
    assert info["n_packets_bad_size"] == 3 and info["n_columns"] == n_cols
    # a packet of the next frame stops the pass; the rest is not taken
    nxt = [bytes(p) for p in encode(S, profile, n_cols, n_rows, cpp, frame, frame_id=8, seed=13)]
    src, col_t, info = assert_same_pass(pkg, profile, cpp, n_cols, n_rows, packets[:1] + nxt + packets[1:])
    assert info["next_frame_pending"] == 1 and info["n_packets"] == 1 and info["frame_id"] == 7
    # nothing at all
    src, col_t, info = assert_same_pass(pkg, profile, cpp, n_cols, n_rows, [])
    assert (src == -1).all() and np.isnan(col_t).all() and info["frame_id"] == -1 and np.isnan(info["t_ref"])


@pytest.mark.parametrize("profile", [RNG19, LEGACY])
def test_times_across_midnight_clamp_to_zero(pkg, S, profile):
    """two timestamps that straddle 86 400 s: the later one wraps to a few microseconds, ts - t_ref is negative and clamps"""
    n_cols, n_rows, cpp = 8, 2, 2
    frame = random_frame(profile, n_cols, n_rows, 1, t0_ns=19_000 * DAY_NS - 3 * 48_828)
    assert frame["ts_ns"][2] < 19_000 * DAY_NS <= frame["ts_ns"][3]
    packets = encode(S, profile, n_cols, n_rows, cpp, frame)
    src, col_t, info = assert_same_pass(pkg, profile, cpp, n_cols, n_rows, packets)
    assert info["t_ref"] > 86399.0 and col_t[1] > 0.0 and col_t[2] > col_t[1] and (col_t[3:] == 0.0).all()
    src, col_t, info = assert_same_pass(pkg, profile, cpp, n_cols, n_rows, packets, t_ref=0.0)
    assert col_t[2] > 86399.0 and 0.0 <= col_t[3] < 1e-3 and col_t[7] > col_t[3]


def test_packet_columns_refusals(pkg, S):
    import ctypes as C
    L = pkg.lib()
    n_cols, n_rows, cpp = 6, 3, 2
    packets = encode(S, RNG19, n_cols, n_rows, cpp, random_frame(RNG19, n_cols, n_rows, 2))
    sizes = np.full(len(packets), packets.shape[1], np.uintp)
    src, col_t, info = np.full(n_cols, -9, np.int32), np.full(n_cols, -9.0, np.float32), pkg.PacketFrameInfo()
    info.n_packets = -9

    def call(profile=RNG19, cpp=cpp, n_cols=n_cols, n_rows=n_rows, p=packets.ctypes.data, s=sizes.ctypes.data, n=len(packets),
             stride=packets.shape[1], t_ref=np.nan, o_src=src.ctypes.data, o_t=col_t.ctypes.data, o_info=C.byref(info)):
        return L.ndt_packet_columns(profile, cpp, n_cols, n_rows, p, s, n, stride, t_ref, o_src, o_t, o_info)

    for bad in (dict(profile=2), dict(profile=-1), dict(cpp=0), dict(n_cols=0), dict(n_rows=0), dict(p=None), dict(s=None),
                dict(stride=packets.shape[1] - 1), dict(stride=0), dict(t_ref=np.inf), dict(t_ref=-np.inf), dict(o_src=None),
                dict(o_t=None), dict(o_info=None), dict(n_cols=65536, n_rows=8192, cpp=1)):     # 2 * 65536 slots of 96 KiB: more than 2^31 dwords
        assert call(**bad) == INVALID_ARG, bad
    assert (src == -9).all() and (col_t == -9.0).all() and info.n_packets == -9           # refused: nothing written
    assert call() == 0 and info.n_packets == len(packets) and (src >= 0).all()
    assert call(p=None, s=None, n=0) == 0 and (src == -1).all()
    assert C.sizeof(pkg.PacketFrameInfo) == 104


# --------------------------------------------------------------------------- 2. the reference's decoder, in arrival order
def reference_decode(profile, cpp, n_cols, n_rows, model, packets, gate, filt):
    """LidarCallback::DecodePacketRng19 (non-AVX branch) / DecodePacketLegacy restated for ONE frame from a fresh callback
    (number_points_ = 0, active_frame_->timestamp = 0): the points it pushes, in its order.  The multiply-add is the exact
    FMA (the reference's AVX path; its scalar path leaves the contraction to the compiler)."""
    header, block, first, size, _ = layout(profile, cpp, n_rows)
    legacy = profile == LEGACY
    x1, y1, z1, x2, y2, z2 = model
    out = {k: [] for k in ("x", "y", "z", "c_id", "m_id", "reflectivity", "signal", "nir", "relative_timestamp")}
    frame_ts, number_points, frame_id = 0.0, 0, None
    step = gate.row_step if gate is not None and gate.row_step > 1 else 1
    for p in packets:
        p = bytes(p)
        if len(p) != size:
            continue
        if not legacy:
            if struct.unpack_from("<H", p, 0)[0] != 1:
                continue
            pid = struct.unpack_from("<H", p, 2)[0]
            if frame_id is None:
                frame_id = pid
            assert pid == frame_id                                            # (one frame: the completion rule is not exercised)
        for col in range(cpp):
            b = header + col * block
            ts = column_ts(struct.unpack_from("<Q", p, b)[0])
            m_id = struct.unpack_from("<H", p, b + 8)[0]
            if m_id >= n_cols:
                continue
            if legacy:
                cid = struct.unpack_from("<H", p, b + 10)[0]
                if frame_id is None:
                    frame_id = cid
                assert cid == frame_id
                if struct.unpack_from("<I", p, b + 16 + 12 * n_rows)[0] != 0xFFFFFFFF:
                    continue
            elif not p[b + 10] & 1:
                continue
            for c_id in range(0, n_rows, step):
                o = b + first + 12 * c_id
                if legacy:
                    rng_mm = struct.unpack_from("<I", p, o)[0] & 0x000FFFFF
                else:
                    rng_mm = (p[o] | (p[o + 1] << 8) | (p[o + 2] << 16)) & 0x0007FFFF
                range_m = np.float32(rng_mm) * np.float32(0.001)
                if gate is not None and gate.use_range and (range_m < np.float32(gate.range_min) or range_m > np.float32(gate.range_max)):
                    continue
                if range_m == 0:
                    continue
                refl = p[o + 4]
                sig, nir = struct.unpack_from("<H", p, o + 6)[0], struct.unpack_from("<H", p, o + 8)[0]
                pt = [fma_f32(range_m, d[m_id, c_id], off[m_id])[()] for d, off in ((x1, x2), (y1, y2), (z1, z2))]
                xyz = np.array([pt], np.float32)
                if not keep_numpy(filt, xyz, np.zeros(1, np.float32), np.array([refl], np.float32))[0]:
                    continue
                rel = max(0.0, ts - frame_ts) if number_points > 0 and frame_ts > 0 else 0.0
                for k, v in zip(out, (pt[0], pt[1], pt[2], c_id, m_id, refl, sig, nir, np.float32(rel))):
                    out[k].append(v)
                number_points += 1
                if number_points == 1:
                    frame_ts = ts
    return out


@pytest.mark.parametrize("profile", [RNG19, LEGACY])
def test_image_route_equals_the_reference_decoder_in_arrival_order(pkg, S, profile):
    """in-order, duplicate-free frames whose first accepted column holds a kept point: NumPy decode + the NumPy unprojection
    and filter of tests/test_gpu_unproject.py give, element for element, what the reference's decoder pushes"""
    n_cols, n_rows, cpp = 24, 5, 4
    model = random_model(n_cols, n_rows, 17)
    filt = pkg.ScanFilter.from_vehicle_box([10.0, -5.0, 0.0], [100.0, 120.0, 140.0], z_band=(-300.0, 100.0), intensity_keep_min=128.0)
    for seed, gate, knobs in ((1, None, {}), (2, pkg.RangeGate(0.5, 400.0, row_step=2), dict(invalid_status=(5, 6), bad_m_id=(9,))),
                              (3, pkg.RangeGate(row_step=3), dict(order=[0, 1, 3, 5]))):
        frame = random_frame(profile, n_cols, n_rows, seed)
        frame["range_mm"][0, 0], frame["reflectivity"][0, 0] = 250_000, 255     # a kept point in the first column: 250 m out, bright
        packets = encode(S, profile, n_cols, n_rows, cpp, frame, seed=seed, **knobs)
        img = decode_numpy(profile, cpp, n_cols, n_rows, list(packets))
        xyz, valid = organised_numpy(model, img["range_mm"], img["col_t"], gate)
        t = np.repeat(img["col_t"], n_rows)
        keep = valid & keep_numpy(filt, xyz, t, img["reflectivity"].ravel().astype(np.float32))
        sel = np.flatnonzero(keep)
        # the precondition, asserted on these inputs: in order, no m_id twice, the first accepted column holds a kept point
        live = np.flatnonzero(img["col_src"] >= 0)
        assert img["info"]["n_columns_overridden"] == 0 and np.all(np.diff(img["col_src"][live]) > 0)
        assert 10 < len(sel) < valid.sum() and sel[0] // n_rows == live[0], (seed, sel[:3], live[:3])
        ref = reference_decode(profile, cpp, n_cols, n_rows, model, list(packets), gate, filt)
        assert len(ref["x"]) == len(sel)
        assert np.array_equal(bits(np.array([ref["x"], ref["y"], ref["z"]], np.float32).T), bits(xyz[sel]))
        assert np.array_equal(ref["m_id"], sel // n_rows) and np.array_equal(ref["c_id"], sel % n_rows)
        for k in ("reflectivity", "signal", "nir"):
            assert np.array_equal(ref[k], img[k].ravel()[sel]), k
        assert np.array_equal(bits(np.array(ref["relative_timestamp"], np.float32)), bits(t[sel]))


# --------------------------------------------------------------------------- 3. sanitizers, stand-alone
def test_packet_host_code_under_asan_ubsan(tmp_path):
    """tests/cpp/sanitize_packets.cpp (its own main) + csrc/ndt_packets.cpp under ASan + UBSan as a child process: packets in
    heap buffers of exactly their size, outputs of exactly n_cols, every disturbance, bytes_each of 0, stride < bytes_each,
    n_rows and cpp at 1.  Never through Python's loader."""
    exe = str(tmp_path / "sanitize_packets")
    csrc = os.path.join(ROOT, "slam-sam_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                        "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                        os.path.join(ROOT, "tests", "cpp", "sanitize_packets.cpp"), os.path.join(csrc, "ndt_packets.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("PASS"), r.stdout[-2000:]


# --------------------------------------------------------------------------- 4. kernel resources
def test_packet_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_packets.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "p.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and name and ("k_decode_packets" in name or "k_gather_u16" in name):
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    kernels = sorted(re.search(r"k_[a-z0-9_]+?(?=E|P|$)", n).group(0) for n in usage)
    print(usage)
    assert len(usage) == 2 and any("k_decode_packets" in n for n in usage) and any("k_gather_u16" in n for n in usage), kernels
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        # LDS: the block's column table, 256 int32, and nothing else -- the figures DESIGN 7j quotes
        assert u["LDS"] == (1024 if "k_decode_packets" in name else 0), (name, u)
