"""Lidar packets decoded on the device (ndt_packet_frame_push, ndt_decode_packet_frame_device, ndt_unproject_packet_frame*,
ndt_keyframe_put_from_packets) against the NumPy decode of tests/test_packets_cpu.py, exactly, and against the range-image
calls fed that decode, bit for bit.  Shapes (n_cols, n_rows, cpp): one packet and less than a block; rows that do not
divide 256; a block that spans 256 columns; 256 pixels and one more; the real row count with two columns per block."""
import os
import subprocess

import numpy as np
import pytest

from test_deskew_cpu import make_trajectory
from test_gpu_deskew import bits, download, f32_knots, read_source
from test_gpu_unproject import device_unproject, filters, random_model
from test_packets_cpu import LEGACY, RNG19, decode_numpy, disturbances, encode, layout, random_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 3, 2), (24, 5, 4), (300, 1, 4), (257, 1, 1), (2, 128, 2), (32, 128, 16)]
PROFILES = [RNG19, LEGACY]
EXTRA = 37                                                   # elements behind every output that must keep their sentinel


@pytest.fixture(scope="module")
def ndt(pkg):
    e = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=50)
    yield e
    e.close()


def set_up(ndt, profile, n_cols, n_rows, cpp, seed=1):
    model = random_model(n_cols, n_rows, seed)
    ndt.setScanModel(*model)
    ndt.setPacketFormat(profile, cpp)
    assert ndt.packetFormat() == (profile, cpp, layout(profile, cpp, n_rows)[3])
    return model


def push_frame(ndt, packets, taken=None):
    ndt.beginPacketFrame()
    assert ndt.pushPackets(packets) == (len(packets) if taken is None else taken)


def device_decode(ndt, hipmem, n_cols, n_rows, refl=True, signal=True, nir=True):
    """decodePacketFrameDevice into arrays EXTRA elements longer than needed -> dict of the images; the sentinels behind
    them are checked here"""
    n = n_cols * n_rows
    spec = dict(range_mm=(np.uint32, n, True), reflectivity=(np.uint8, n, refl), signal=(np.uint16, n, signal),
                nir=(np.uint16, n, nir), col_t=(np.float32, n_cols, True))
    sentinel = dict(range_mm=0xDEADBEEF, reflectivity=0xA7, signal=0xBEEF, nir=0xFACE, col_t=-7.0)
    d = {k: hipmem.upload(np.full(m + EXTRA, sentinel[k], t)) if on else None for k, (t, m, on) in spec.items()}
    ndt.decodePacketFrameDevice(d["range_mm"], d["reflectivity"], d["signal"], d["nir"], d["col_t"])
    out = {}
    for k, (t, m, on) in spec.items():
        if on:
            raw = download(hipmem, d[k], m + EXTRA, t)
            assert np.all(raw[m:] == np.array(sentinel[k], t)), k
            out[k] = raw[:m]
    return out


def assert_image(got, want, n_cols, n_rows):
    for k in ("range_mm", "reflectivity", "signal", "nir"):
        if k in got:
            assert np.array_equal(got[k].reshape(n_cols, n_rows), want[k]), k
    assert np.array_equal(bits(got["col_t"]), bits(want["col_t"]))


# ---- 1. decode equals NumPy decode ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("n_cols,n_rows,cpp", SHAPES)
def test_decode_equals_numpy_decode(pkg, S, ndt, hipmem, profile, n_cols, n_rows, cpp):
    set_up(ndt, profile, n_cols, n_rows, cpp)
    frame = random_frame(profile, n_cols, n_rows, 100 + n_cols + n_rows)
    for name, knobs in disturbances(profile, n_cols, cpp).items():
        packets = encode(S, profile, n_cols, n_rows, cpp, frame, seed=5, garbage=True, **knobs)
        want = decode_numpy(profile, cpp, n_cols, n_rows, list(packets))
        # (LEGACY with one column per packet: the column of another frame id IS a packet of the next frame and stops the push)
        push_frame(ndt, packets, taken=want["info"]["n_packets"])
        if want["info"]["n_columns"] == 0:                   # (two columns, both with an invalid status)
            with pytest.raises(pkg.NdtError) as e:
                device_decode(ndt, hipmem, n_cols, n_rows)
            assert "no accepted column" in str(e.value) and name == "invalid status" and n_cols == 2
            continue
        got = device_decode(ndt, hipmem, n_cols, n_rows)
        assert_image(got, want, n_cols, n_rows)
        info = ndt.packetFrameInfo()
        for k, v in want["info"].items():
            assert info[k] == v or (np.isnan(v) and np.isnan(info[k])), (name, k, info[k], v)
        if name == "in order":
            # the garbage bits are in the payloads and not in the image; the image is the frame
            assert (np.frombuffer(packets.tobytes(), np.uint8) != 0).mean() > 0.9
            for k in ("range_mm", "reflectivity", "signal", "nir"):
                assert np.array_equal(got[k].reshape(n_cols, n_rows), frame[k]), k
            # the nullable outputs, each left out
            for off in ("refl", "signal", "nir"):
                assert_image(device_decode(ndt, hipmem, n_cols, n_rows, **{off: False}), want, n_cols, n_rows)
        hipmem.free_all()


# ---- 2. the packet forms equal the range-image forms ------------------------------------------------------------------------
def device_unproject_packets(ndt, hipmem, n, traj=None, gate=None, filt=None, fill=-1.0, extras=True, index=True):
    init = np.full(n + EXTRA, fill, np.float32)
    o = [hipmem.upload(init) for _ in range(5)]
    didx = hipmem.upload(np.full(n + EXTRA, -7, np.int32)) if index else None
    dsig, dnir = (hipmem.upload(np.full(n + EXTRA, 0xBEEF, np.uint16)) for _ in range(2)) if extras else (None, None)
    kt, kp = (None, None) if traj is None else traj
    m = ndt.unprojectPacketFrameDevice(o[0], o[1], o[2], n, knot_t=kt, knot_poses=kp, gate=gate, filter=filt, o_intensity=o[3], o_t=o[4],
                                       d_index=didx, d_signal=dsig, d_nir=dnir)
    raw = [download(hipmem, p, n + EXTRA) for p in o]
    assert all(np.all(a[m:] == fill) for a in raw)                          # nothing behind the points written
    res = dict(xyz=np.stack(raw[:3], 1)[:m], intensity=raw[3][:m], t=raw[4][:m], m=m)
    if index:
        ridx = download(hipmem, didx, n + EXTRA, np.int32)
        assert np.all(ridx[m:] == -7)
        res["index"] = ridx[:m]
    if extras:
        rs, rn = download(hipmem, dsig, n + EXTRA, np.uint16), download(hipmem, dnir, n + EXTRA, np.uint16)
        assert np.all(rs[m:] == 0xBEEF) and np.all(rn[m:] == 0xBEEF)
        res["signal"], res["nir"] = rs[:m], rn[:m]
    return res


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("n_cols,n_rows,cpp", SHAPES)
def test_packet_forms_equal_range_image_forms(pkg, S, ndt, hipmem, profile, n_cols, n_rows, cpp):
    n = n_cols * n_rows
    set_up(ndt, profile, n_cols, n_rows, cpp, seed=7)
    k = (n_cols + cpp - 1) // cpp
    knobs = dict(invalid_status=(1,), duplicate=(0,), order=list(range(k))[::-1] if k < 3 else [0] + list(range(2, k)))   # (three packets and more: packet 1 is lost)
    named = filters(pkg)
    # no filter; the zeroed one; a vehicle box around the sensor, a z band and a reflectivity threshold behind a range gate
    # (ranges reach 524 m and 1048 m: a box of 100 m leaves most points, the threshold about half of those above the band)
    near = pkg.ScanFilter.from_vehicle_box([10.0, -5.0, 0.0], [100.0, 120.0, 140.0], z_band=(-300.0, 100.0), intensity_keep_min=128.0)
    cases = [(None, None), (named[1][1], None), (near, pkg.RangeGate(0.5, 450.0, row_step=2 if n_rows > 1 else 0))]
    for n_knots in (0, 2, 64):
        traj = None
        span = 0.1
        if n_knots:
            kt, kp = make_trajectory(n_knots, 70 + n_knots)
            traj = (f32_knots(kt), kp)
            span = float(traj[0][-1])
        # column times from before the first knot... the first accepted column is time 0; the last lies behind the last knot
        frame = random_frame(profile, n_cols, n_rows, 200 + n + n_knots, dt_ns=max(1, int(1.2e9 * span / n_cols)))
        packets = encode(S, profile, n_cols, n_rows, cpp, frame, seed=9, **knobs)
        img = decode_numpy(profile, cpp, n_cols, n_rows, list(packets))
        push_frame(ndt, packets)
        for filt, gate in cases:
            what = (n_knots, filt is not None, gate is not None)
            want = device_unproject(ndt, hipmem, img["range_mm"], img["reflectivity"], img["col_t"], traj=traj, gate=gate, filt=filt)
            assert want["m"] == n if filt is None else (want["m"] < n and (want["m"] > 0 or n < 50)), what
            got = device_unproject_packets(ndt, hipmem, n, traj=traj, gate=gate, filt=filt)
            assert got["m"] == want["m"], what
            for key in ("xyz", "intensity", "t"):
                assert np.array_equal(bits(got[key]), bits(want[key])), what + (key,)
            assert np.array_equal(got["index"], want["index"]), what
            assert np.array_equal(got["signal"], img["signal"].ravel()[want["index"]]), what
            assert np.array_equal(got["nir"], img["nir"].ravel()[want["index"]]), what
            # without an index output the gather goes through the handle's own; without extras nothing else changes
            lean = device_unproject_packets(ndt, hipmem, n, traj=traj, gate=gate, filt=filt, index=False)
            assert np.array_equal(lean["signal"], got["signal"]) and np.array_equal(lean["nir"], got["nir"]), what
            bare = device_unproject_packets(ndt, hipmem, n, traj=traj, gate=gate, filt=filt, extras=False)
            assert np.array_equal(bits(bare["xyz"]), bits(want["xyz"])), what
            # the host form against ndt_unproject fed the decoded image
            kw = dict(knot_t=None if traj is None else traj[0], knot_poses=None if traj is None else traj[1], gate=gate, filter=filt)
            h_cloud, h_t, h_idx = ndt.unproject(img["range_mm"], img["reflectivity"], img["col_t"], with_t=True, with_index=True, **kw)
            cloud, tt, idx, sig, nir = ndt.unprojectPacketFrame(with_t=True, with_index=True, with_signal=True, with_nir=True, **kw)
            assert cloud.shape == h_cloud.shape == (want["m"], 4) and np.array_equal(bits(cloud), bits(h_cloud)), what
            assert np.array_equal(bits(tt), bits(h_t)) and np.array_equal(idx, h_idx), what
            assert np.array_equal(sig, img["signal"].ravel()[h_idx]) and np.array_equal(nir, img["nir"].ravel()[h_idx]), what
            only_nir = ndt.unprojectPacketFrame(with_nir=True, **kw)
            assert np.array_equal(bits(only_nir[0]), bits(h_cloud)) and np.array_equal(only_nir[1], nir), what
            hipmem.free_all()


# ---- 3. the keyframe form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", PROFILES)
def test_keyframe_from_packets_is_the_keyframe_from_ranges(pkg, S, ndt, hipmem, profile):
    n_cols, n_rows, cpp = 24, 5, 4
    set_up(ndt, profile, n_cols, n_rows, cpp, seed=3)
    kt, kp = make_trajectory(5, 13)
    kt = f32_knots(kt)
    frame = random_frame(profile, n_cols, n_rows, 31, dt_ns=int(1e9 * kt[-1] / n_cols))
    packets = encode(S, profile, n_cols, n_rows, cpp, frame, seed=2, order=[0, 1, 2, 4, 5], invalid_status=(3,))
    img = decode_numpy(profile, cpp, n_cols, n_rows, list(packets))
    push_frame(ndt, packets)
    f = pkg.ScanFilter.from_vehicle_box([0.0, 0.0, 0.0], [300.0, 300.0, 300.0], z_band=(-400.0, 100.0), intensity_keep_min=200.0)
    for filt, gate, traj in ((None, None, False), (f, pkg.RangeGate(1.0, 500.0, row_step=2), True)):
        kw = dict(knot_t=kt if traj else None, knot_poses=kp if traj else None, gate=gate, filter=filt)
        kept_r = ndt.putKeyframeFromRanges(41, img["range_mm"], img["reflectivity"], img["col_t"], **kw)
        ndt.setInputSourceFromKeyframe(41)
        want = read_source(pkg, ndt)
        _, idx = ndt.unproject(img["range_mm"], img["reflectivity"], img["col_t"], with_index=True,
                               **dict(kw, filter=filt if filt is not None else pkg.ScanFilter()))
        kept_p, sig, nir = ndt.putKeyframeFromPackets(42, with_signal=True, with_nir=True, **kw)
        assert kept_p == kept_r == len(idx) and 0 < kept_p < n_cols * n_rows
        ndt.setInputSourceFromKeyframe(42)
        got = read_source(pkg, ndt)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
        assert np.array_equal(sig, img["signal"].ravel()[idx]) and np.array_equal(nir, img["nir"].ravel()[idx])
        # replacing the keyframe that is the viewed source unsets the source, as ndt_keyframe_put does
        assert ndt.putKeyframeFromPackets(42, **kw) == kept_p
        assert ndt.sourceSize() == 0
    ndt.eraseKeyframe(41)
    ndt.eraseKeyframe(42)


# ---- 4. push in pieces ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", PROFILES)
def test_push_in_pieces(pkg, S, ndt, hipmem, profile):
    n_cols, n_rows, cpp = 24, 5, 4
    set_up(ndt, profile, n_cols, n_rows, cpp)
    a = encode(S, profile, n_cols, n_rows, cpp, random_frame(profile, n_cols, n_rows, 1), frame_id=7, seed=1,
               order=[3, 0, 1, 2, 5], duplicate=(1,), invalid_status=(2,))
    b = encode(S, profile, n_cols, n_rows, cpp, random_frame(profile, n_cols, n_rows, 2, t0_ns=1_700_000_100 * 10 ** 9), frame_id=8, seed=2)
    want_a, want_b = (decode_numpy(profile, cpp, n_cols, n_rows, list(p)) for p in (a, b))
    push_frame(ndt, a)
    assert_image(device_decode(ndt, hipmem, n_cols, n_rows), want_a, n_cols, n_rows)
    info_all = ndt.packetFrameInfo()
    # one packet per call, a bytes payload each
    ndt.beginPacketFrame()
    for p in a:
        assert ndt.pushPackets([p.tobytes()]) == 1
    assert_image(device_decode(ndt, hipmem, n_cols, n_rows), want_a, n_cols, n_rows)
    assert ndt.packetFrameInfo() == info_all
    # split at every position; the image after the first part is the decode of that part
    for s in range(len(a) + 1):
        ndt.beginPacketFrame()
        assert ndt.pushPackets(a[:s]) == s and ndt.pushPackets(a[s:]) == len(a) - s
        assert_image(device_decode(ndt, hipmem, n_cols, n_rows), want_a, n_cols, n_rows)
        hipmem.free_all()
    ndt.beginPacketFrame()
    ndt.pushPackets(a[:2])
    assert_image(device_decode(ndt, hipmem, n_cols, n_rows), decode_numpy(profile, cpp, n_cols, n_rows, list(a[:2])), n_cols, n_rows)
    ndt.pushPackets(a[2:])
    assert_image(device_decode(ndt, hipmem, n_cols, n_rows), want_a, n_cols, n_rows)
    # the next frame's first packet stops the push
    ndt.beginPacketFrame()
    both = np.concatenate([a, b])
    assert ndt.pushPackets(both) == len(a)
    info = ndt.packetFrameInfo()
    assert info["next_frame_pending"] == 1 and info["frame_id"] == 7 and info["n_packets"] == len(a)
    assert_image(device_decode(ndt, hipmem, n_cols, n_rows), want_a, n_cols, n_rows)
    ndt.beginPacketFrame()
    assert ndt.packetFrameInfo()["frame_id"] == -1 and ndt.packetFrameInfo()["next_frame_pending"] == 0
    assert ndt.pushPackets(both[len(a):]) == len(b)
    assert_image(device_decode(ndt, hipmem, n_cols, n_rows), want_b, n_cols, n_rows)
    assert ndt.packetFrameInfo()["frame_id"] == 8
    # overfull by one packet: refused, nothing of the call taken, the frame in progress intact
    capacity = 2 * ((n_cols + cpp - 1) // cpp)
    twice = np.concatenate([b, b])
    assert len(twice) == capacity
    ndt.beginPacketFrame()
    assert ndt.pushPackets(twice) == capacity
    before = ndt.packetFrameInfo()
    for more in (b[:1], np.concatenate([a[:0], b[3:5]])):
        with pytest.raises(pkg.NdtError) as e:
            ndt.pushPackets(more)
        assert e.value.code == -1 and "frame overfull" in str(e.value)
        assert ndt.packetFrameInfo() == before
    assert_image(device_decode(ndt, hipmem, n_cols, n_rows), decode_numpy(profile, cpp, n_cols, n_rows, list(twice)), n_cols, n_rows)
    ndt.beginPacketFrame()
    assert ndt.pushPackets(b) == len(b)
    before = ndt.packetFrameInfo()
    with pytest.raises(pkg.NdtError):
        ndt.pushPackets(np.concatenate([b, b[:1]]))                          # the call's LAST packet is the one too many
    assert ndt.packetFrameInfo() == before
    # rejected packets are taken and need no slot
    short = [p.tobytes()[:-4] for p in b]
    assert ndt.pushPackets(short) == len(short) and ndt.packetFrameInfo()["n_packets_bad_size"] == len(short)
    assert ndt.pushPackets(b) == len(b)
    assert_image(device_decode(ndt, hipmem, n_cols, n_rows), want_b, n_cols, n_rows)


# ---- 5. refusals and state ------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_name_the_cause(pkg, S, ndt, hipmem):
    profile, n_cols, n_rows, cpp = RNG19, 6, 50, 3
    n = n_cols * n_rows
    packets = encode(S, profile, n_cols, n_rows, cpp, random_frame(profile, n_cols, n_rows, 4))
    outs = [hipmem.upload(np.full(n, -1.0, np.float32)) for _ in range(5)]
    d_idx = hipmem.upload(np.full(n, -7, np.int32))
    d_sig, d_nir = (hipmem.upload(np.full(n, 0xBEEF, np.uint16)) for _ in range(2))
    d_rng, d_refl = hipmem.upload(np.full(n, 0xDEADBEEF, np.uint32)), hipmem.upload(np.full(n, 0xA7, np.uint8))
    d_t = hipmem.upload(np.full(n_cols, -7.0, np.float32))
    cloud = np.full((n, 4), -1.0, np.float32)

    def untouched():
        assert all(np.all(download(hipmem, p, n) == -1.0) for p in outs) and np.all(download(hipmem, d_idx, n, np.int32) == -7)
        assert np.all(download(hipmem, d_sig, n, np.uint16) == 0xBEEF) and np.all(download(hipmem, d_nir, n, np.uint16) == 0xBEEF)
        assert np.all(download(hipmem, d_rng, n, np.uint32) == 0xDEADBEEF) and np.all(download(hipmem, d_refl, n, np.uint8) == 0xA7)
        assert np.all(download(hipmem, d_t, n_cols) == -7.0) and np.all(cloud == -1.0)

    def refused(cause, call):
        with pytest.raises(pkg.NdtError) as e:
            call()
        assert e.value.code == -1 and cause in str(e.value), (cause, str(e.value))
        untouched()

    def every_call(cause, **kw):
        archived = ndt.keyframeCount()
        refused(cause, lambda: ndt.decodePacketFrameDevice(d_rng, d_refl, d_sig, d_nir, d_t))
        for filt in (None, pkg.ScanFilter()):
            refused(cause, lambda: ndt.unprojectPacketFrameDevice(outs[0], outs[1], outs[2], n, filter=filt, o_intensity=outs[3],
                                                                  o_t=outs[4], d_index=d_idx, d_signal=d_sig, d_nir=d_nir, **kw))
            refused(cause, lambda: ndt.unprojectPacketFrame(filter=filt, with_signal=True, **kw))
            refused(cause, lambda: ndt.putKeyframeFromPackets(993, filter=filt, **kw))
        assert ndt.keyframeCount() == archived

    ndt.clearScanModel()
    assert ndt.packetFormat() == (-1, 0, 0)
    refused("no scan model", lambda: ndt.setPacketFormat(profile, cpp))
    refused("no scan model", ndt.beginPacketFrame)
    refused("no scan model", lambda: ndt.pushPackets(packets))
    every_call("no scan model")
    ndt.setScanModel(*random_model(n_cols, n_rows, 5))
    refused("no packet format", ndt.beginPacketFrame)
    refused("no packet format", lambda: ndt.pushPackets(packets))
    every_call("no packet format")
    for bad in ((2, cpp), (-1, cpp), (profile, 0), (profile, -3)):
        refused("packet format", lambda: ndt.setPacketFormat(*bad))
    assert ndt.packetFormat() == (-1, 0, 0)
    ndt.setPacketFormat(profile, cpp)
    ndt.beginPacketFrame()
    every_call("no accepted column")
    assert ndt.pushPackets([p.tobytes()[:-1] for p in packets]) == len(packets)   # taken, all rejected
    every_call("no accepted column")
    import ctypes as C
    taken = C.c_size_t(9)
    sizes = np.full(len(packets), packets.shape[1], np.uintp)
    L = pkg.lib()
    assert L.ndt_packet_frame_push(ndt._h, packets.ctypes.data, sizes.ctypes.data, len(packets), packets.shape[1] - 1, C.byref(taken)) == -1
    assert "stride_bytes" in L.ndt_last_error(ndt._h).decode() and taken.value == 0
    assert L.ndt_packet_frame_push(ndt._h, None, sizes.ctypes.data, len(packets), packets.shape[1], C.byref(taken)) == -1
    assert L.ndt_packet_frame_push(ndt._h, packets.ctypes.data, sizes.ctypes.data, len(packets), packets.shape[1], None) == -1
    assert ndt.packetFrameInfo()["n_packets_accepted"] == 0
    assert ndt.pushPackets(packets) == len(packets)
    # every refusal of the calls they stand for
    kt, kp = make_trajectory(3, 8)
    every = lambda cause, **kw: [refused(cause, lambda: ndt.unprojectPacketFrameDevice(   # noqa: E731
        outs[0], outs[1], outs[2], n, filter=filt, o_intensity=outs[3], o_t=outs[4], d_index=d_idx, d_signal=d_sig, d_nir=d_nir, **kw))
        for filt in (None, pkg.ScanFilter())] + [refused(cause, lambda: ndt.unprojectPacketFrame(with_nir=True, **kw)),
                                                 refused(cause, lambda: ndt.putKeyframeFromPackets(994, with_signal=True, **kw))]
    archived = ndt.keyframeCount()
    every("row_step", gate=pkg.RangeGate(row_step=-1))
    every("range_min", gate=pkg.RangeGate(2.0, 1.0))
    every("strictly increasing", knot_t=kt[::-1].copy(), knot_poses=kp)
    bad_pose = kp.copy()
    bad_pose[1, 0, 3] = np.inf
    every("non-finite pose entry", knot_t=kt, knot_poses=bad_pose)
    assert ndt.keyframeCount() == archived
    for filt in (None, pkg.ScanFilter()):
        dev = lambda **kw: ndt.unprojectPacketFrameDevice(**dict(dict(ox=outs[0], oy=outs[1], oz=outs[2], cap=n, filter=filt,   # noqa: E731
                                                                      o_intensity=outs[3], o_t=outs[4], d_index=d_idx, d_signal=d_sig,
                                                                      d_nir=d_nir), **kw))
        refused("NULL", lambda: dev(oy=None))
        refused("overlap", lambda: dev(oz=outs[0]))
        refused("overlap", lambda: dev(d_signal=outs[1] + 2))
        refused("overlap", lambda: dev(d_nir=d_idx))
        refused("overlap", lambda: dev(d_nir=d_sig + 2 * n - 2))
    refused(str(n), lambda: ndt.unprojectPacketFrameDevice(outs[0], outs[1], outs[2], n - 1, d_signal=d_sig))   # organised, cap below n
    assert ndt.last_unproject_count == n
    refused("overlap", lambda: ndt.decodePacketFrameDevice(d_rng, d_refl, d_sig, d_sig, d_t))
    refused("NULL", lambda: ndt.decodePacketFrameDevice(None, d_refl, d_sig, d_nir, d_t))
    refused("NULL", lambda: ndt.decodePacketFrameDevice(d_rng, d_refl, d_sig, d_nir, None))
    n_out = C.c_size_t(0)
    rc = L.ndt_unproject_packet_frame(ndt._h, None, None, None, 0, None, None, cloud.ctypes.data, 10, -1, None, None, None, None, n, C.byref(n_out))
    assert rc == -1 and "layout" in L.ndt_last_error(ndt._h).decode()
    rc = L.ndt_unproject_packet_frame(ndt._h, None, None, None, 0, None, None, None, 16, 12, None, None, None, None, n, C.byref(n_out))
    assert rc == -1 and "output cloud" in L.ndt_last_error(ndt._h).decode()
    sig = np.full(n, 0xBEEF, np.uint16)
    rc = L.ndt_unproject_packet_frame(ndt._h, None, None, None, 0, None, C.byref(pkg.ScanFilter()), cloud.ctypes.data, 16, 12, None, None,
                                      sig.ctypes.data, None, 5, C.byref(n_out))
    assert rc == -1 and n_out.value > 5 and str(n_out.value) in L.ndt_last_error(ndt._h).decode() and np.all(sig == 0xBEEF)
    untouched()
    # ... and with nothing wrong every call goes through
    ndt.decodePacketFrameDevice(d_rng, d_refl, d_sig, d_nir, d_t)
    assert ndt.unprojectPacketFrameDevice(outs[0], outs[1], outs[2], n, o_intensity=outs[3], o_t=outs[4], d_index=d_idx, d_signal=d_sig,
                                          d_nir=d_nir) == n
    # a new model drops the format and the frame
    ndt.setScanModel(*random_model(n_cols, n_rows, 6))
    assert ndt.packetFormat() == (-1, 0, 0)
    with pytest.raises(pkg.NdtError) as e:
        ndt.unprojectPacketFrame()
    assert "no packet format" in str(e.value)
    ndt.setPacketFormat(profile, cpp)
    with pytest.raises(pkg.NdtError) as e:
        ndt.unprojectPacketFrame()
    assert "no accepted column" in str(e.value)


def test_packet_calls_leave_the_engine_state_alone(pkg, S, ndt, hipmem):
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
    profile, n_cols, n_rows, cpp = LEGACY, 40, 64, 8
    set_up(ndt, profile, n_cols, n_rows, cpp, seed=2)
    kt, kp = make_trajectory(5, 13)
    packets = encode(S, profile, n_cols, n_rows, cpp, random_frame(profile, n_cols, n_rows, 14, dt_ns=int(1e9 * kt[-1] / n_cols)))
    push_frame(ndt, packets)
    device_decode(ndt, hipmem, n_cols, n_rows)
    ndt.unprojectPacketFrame()
    ndt.unprojectPacketFrame(kt, kp, filter=pkg.ScanFilter(), gate=pkg.RangeGate(1.0, 500.0, row_step=2), with_signal=True, with_nir=True)
    device_unproject_packets(ndt, hipmem, n_cols * n_rows, traj=(kt, kp), filt=pkg.ScanFilter())
    with pytest.raises(pkg.NdtError):
        ndt.unprojectPacketFrame(kt[::-1].copy(), kp)
    with pytest.raises(pkg.NdtError):
        ndt.putKeyframeFromPackets(71, kt[::-1].copy(), kp)
    ndt.beginPacketFrame()
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


# ---- 6. the C++ face ------------------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, tmp_path):
    """tests/cpp/test_packets.cpp against the API mocks, built with the g++ line tests/test_gpu_unproject.py uses."""
    d = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "test_packets")
    lib = os.path.join(ROOT, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(ROOT, "include", "compat"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(d, "test_packets.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "packets: PASS" in p.stdout
