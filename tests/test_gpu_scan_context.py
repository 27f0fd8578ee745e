"""Scan Context place recognition on the device (ndt_scan_context*) against the NumPy restatement of the header's rules
(test_scan_context_cpu.scan_context_numpy / scan_context_match_numpy), bit for bit: descriptors and counts of the host,
device and keyframe forms; distance (as uint64 bits), shift and columns of every bank entry; the bank's state rules; and
one loop closure end to end -- the matched shift as the initial guess of an align that the identity guess does not solve,
held to the CPU oracle's align from the same guess with the tolerances of tests/test_gpu_parity.py (1 mm, 0.1 mrad).
The sector table is read back through ndt_scan_context_sector_table, never recomputed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_scan_context_cpu import (CLOSURE_KW, CLOSURE_QUERY, CLOSURE_RESOLUTION, CLOSURE_TOL_M, CLOSURE_TOL_RAD, N_PLACES,
                                   closure_case, place_descriptors, places, scan_context_match_numpy, scan_context_numpy)
from test_gpu_map_target import code_of

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
ALIGN_TOL_M, ALIGN_TOL_RAD = 1e-3, 1e-4
SHAPES = [(20, 60), (1, 3), (32, 128), (20, 64), (20, 65)]
PREFIXES = (0, 1, 63, 64, 65, 256, 257)                                      # a lone lane, the wave edge, the block edge, two blocks


def engine(pkg, **kw):
    return pkg.NormalDistributionsTransform(device_id=0, **dict(dict(resolution=1.0), **kw))


def download(hipmem, ptr, shape, dtype):
    a = np.zeros(shape, dtype)
    assert hipmem.rt.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0               # hipMemcpyDeviceToHost
    return a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def hand_made(dirs, R, max_radius=80.0):
    """the points at which the rule can go wrong: on the sector directions, at the origin, on the ring edges, at the
    radius gate, non-finite, at and below height zero"""
    f = np.float32
    rows = []
    for radius in (f(7.0), f(33.3), f(79.5)):
        for k in range(len(dirs)):
            rows.append([dirs[k, 0] * radius, dirs[k, 1] * radius, f(0.25) * f(k % 7)])        # on or next to a sector boundary
    rows += [[0, 0, 1], [0, 0, -3], [-0.0, 0.0, 2], [0, 1e-30, 1], [1e-30, 0, 1], [-1e-30, -1e-30, 1]]   # the origin, and almost
    edge = max_radius / R
    for i in range(1, R + 1):                                                 # ring edges (4, 0), (8, 0), ... (0, -76) at 80 m / 20
        e = f(i * edge)
        rows += [[e, 0, 1], [0, -e, 1.5], [np.nextafter(e, f(0)), 0, 0.5], [0, np.nextafter(e, f(1e9)), 0.75]]
    rows += [[4, 0, 1], [8, 0, 1], [0, -76, 1]]
    m = f(max_radius)
    rows += [[m, 0, 5], [0, m, 5], [np.nextafter(m, f(0)), 0, 5], [0, -np.nextafter(m, f(0)), 6], [m * f(0.6), m * f(0.8), 7],
             [np.nextafter(m, f(1e9)), 0, 5], [3e38, 3e38, 1], [1e20, -1e20, 1]]
    rows += [[np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.inf, 1, 1], [1, -np.inf, 1], [1, 1, np.inf], [1, 1, -np.inf],
             [np.nan, np.nan, np.nan]]
    rows += [[5, 5, -2], [5, -5, -2.5], [-5, 5, -0.0], [-5, -5, -1.9999999], [12, 1, -2], [12, 1.01, -100], [20, 3, 3e38], [20, 3.1, -3e38]]
    return np.array(rows, dtype=np.float32)


def crowd(n=10000):
    """ten thousand points in one bin (ring 2, sector 0 of the default shape), heights spread"""
    rng = np.random.default_rng(8)
    return np.stack([rng.uniform(10.0, 10.5, n), rng.uniform(0.2, 0.6, n), rng.uniform(-3.0, 6.0, n)], 1).astype(np.float32)


def random_cloud(n, seed=4):
    rng = np.random.default_rng(seed)
    r, a = rng.uniform(0.0, 95.0, n), rng.uniform(0.0, 2 * np.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-4.0, 9.0, n)], 1).astype(np.float32)


def all_forms(pkg, ndt, hipmem, cloud, shape):
    """[(desc, count)] of the host, device and keyframe forms"""
    R, S = shape
    out = [pkg.scanContext(ndt, cloud, with_count=True)]
    n = len(cloud)
    soa = [hipmem.upload(np.ascontiguousarray(cloud[:, a])) if n else None for a in range(3)]
    d_desc = hipmem.upload(np.full((R, S), 7.0, np.float32))
    d_count = hipmem.upload(np.full((R, S), 7, np.int32))
    pkg.scanContextDevice(ndt, soa[0], soa[1], soa[2], n, d_desc, d_count)
    out.append((download(hipmem, d_desc, (R, S), np.float32), download(hipmem, d_count, (R, S), np.int32)))
    pkg.scanContextDevice(ndt, soa[0], soa[1], soa[2], n, d_desc, None)                            # the count is optional
    assert same_bits(download(hipmem, d_desc, (R, S), np.float32), out[-1][0])
    ndt.putKeyframe(900, cloud)
    out.append(pkg.scanContextKeyframe(ndt, 900, with_count=True))
    assert same_bits(pkg.scanContextBankGet(ndt, 900), out[-1][0])
    assert same_bits(pkg.scanContextKeyframe(ndt, 900), out[-1][0])                                # without the count
    return out


# ---- 1. descriptor and count bits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_descriptor_bits_equal_the_restatement(pkg, hipmem, shape):
    R, S = shape
    ndt = engine(pkg)
    dirs = pkg.scanContextSectorTable(S)
    hand = hand_made(dirs, R)
    mixed = np.concatenate([hand, random_cloud(400)])
    mixed = mixed[np.random.default_rng(1).permutation(len(mixed))]
    clouds = [("prefix %d" % n, mixed[:n]) for n in PREFIXES]
    clouds += [("hand-made + crowd", np.concatenate([hand, crowd(), random_cloud(3000, seed=6)])), ("scan", places()["bank"][4])]
    assert len(clouds[-1][1]) > 8000
    checked = 0
    for z_sign in (1.0, -1.0):
        for min_pts in (1, 3):
            prm = dict(n_rings=R, n_sectors=S, z_sign=z_sign, min_points_per_bin=min_pts)
            pkg.setScanContextParams(ndt, **prm)
            assert pkg.getScanContextParams(ndt) == dict(prm, max_radius=80.0, lift=2.0)
            for name, cloud in clouds:
                if name == "scan" and (z_sign, min_pts) not in ((1.0, 1), (-1.0, 3)):
                    continue
                want = scan_context_numpy(cloud, dirs, max_radius=80.0, lift=2.0, **prm)
                for form, got in zip(("host", "device", "keyframe"), all_forms(pkg, ndt, hipmem, cloud, shape)):
                    assert same_bits(got[1], want[1]), (name, form, prm, "count")
                    assert same_bits(got[0], want[0]), (name, form, prm, "desc")
                checked += 1
                if len(cloud) == 0:
                    assert not want[0].any() and not want[1].any()
                if name == "hand-made + crowd" and shape == (20, 60) and min_pts == 1:
                    assert want[1][2, 0] >= 10000 and int(want[1].sum()) < len(cloud)              # the crowd's bin; some are skipped
                    assert (want[0][want[1] > 0] == 0).any()                                       # occupied bins of height <= 0
    assert checked == 4 * (len(clouds) - 1) + 2
    hipmem.free_all()


def test_other_radius_and_lift(pkg, hipmem):
    ndt = engine(pkg)
    dirs = pkg.scanContextSectorTable(60)
    cloud = np.concatenate([hand_made(dirs, 7, max_radius=33.3), random_cloud(2000)])
    for prm in (dict(n_rings=7, max_radius=33.3, lift=-1.25), dict(n_rings=7, max_radius=1e-3, lift=0.0),
                dict(n_rings=32, max_radius=3e38, lift=3e38, z_sign=-1.0)):
        pkg.setScanContextParams(ndt, **prm)
        want = scan_context_numpy(cloud, dirs, **dict(dict(n_sectors=60), **prm))
        for got in all_forms(pkg, ndt, hipmem, cloud, (prm["n_rings"], 60)):
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), prm


# ---- the 13 places on the device ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(pkg):
    """one engine with the 13 bank scans archived as keyframes 0 .. 12 and the 13 queries as 100 .. 112, their descriptors
    in the bank under the same ids"""
    p = places()
    ndt = engine(pkg)
    for i in range(N_PLACES):
        ndt.putKeyframe(i, p["bank"][i])
        ndt.putKeyframe(100 + i, p["query"][i])
    bank = np.stack([pkg.scanContextKeyframe(ndt, i) for i in range(N_PLACES)])
    query = np.stack([pkg.scanContextKeyframe(ndt, 100 + i) for i in range(N_PLACES)])
    return dict(ndt=ndt, bank=bank, query=query)


def test_places_on_the_device(pkg, rig):
    """the keyframe descriptors are the restatement's, and the device finds what test_the_rule_recognises_places finds"""
    ndt = rig["ndt"]
    want_bank, want_query = place_descriptors()
    assert same_bits(rig["bank"], want_bank) and same_bits(rig["query"], want_query)
    assert pkg.scanContextBankCount(ndt) == 2 * N_PLACES
    p = places()
    for i in range(N_PLACES):
        m = pkg.scanContextMatchKeyframe(ndt, 100 + i)
        assert m["ids"].tolist() == list(range(N_PLACES)) + list(range(100, 100 + N_PLACES))
        d, s, c = scan_context_match_numpy(want_query[i], np.concatenate([want_bank, want_query]))
        assert same_bits(m["distance"].view(np.uint64), d.view(np.uint64)) and same_bits(m["shift"], s) and same_bits(m["columns"], c)
        assert int(np.argmin(m["distance"][:N_PLACES])) == i
        assert m["shift"][i] in (p["k"][i], (p["k"][i] + 30) % 60)
        assert m["shift"][N_PLACES + i] == 0 and abs(m["distance"][N_PLACES + i]) < 1e-12         # the query's own entry
        h = pkg.scanContextMatch(ndt, pkg.scanContextBankGet(ndt, 100 + i))                       # the same query through the host
        for k in ("ids", "distance", "shift", "columns"):
            assert same_bits(m[k], h[k]), k


# ---- 2. match bits ------------------------------------------------------------------------------------------------------
def sparse(rng, R, S, fill):
    return (rng.uniform(0.0, 12.0, (R, S)) * (rng.random((R, S)) < fill)).astype(np.float32)


def special_entries(R, S, seed=12):
    """named descriptors: all zero, empty columns, periodic in the sectors, one column, one bin, huge and tiny values"""
    rng = np.random.default_rng(seed)
    gaps = sparse(rng, R, S, 0.7)
    gaps[:, rng.random(S) < 0.5] = 0.0
    period = next(q for q in (4, 5, 3, 2, 1) if S % q == 0)
    periodic = np.tile(sparse(rng, R, period, 0.9) + np.float32(0.5), (1, S // period))
    one_col = np.zeros((R, S), np.float32)
    one_col[:, S // 2] = 1.0 + rng.random(R).astype(np.float32)
    one_bin = np.zeros((R, S), np.float32)
    one_bin[R - 1, S - 1] = 3.0
    scaled = sparse(rng, R, S, 0.5)
    return dict(zero=np.zeros((R, S), np.float32), gaps=gaps, periodic=periodic, one_col=one_col, one_bin=one_bin,
                huge=scaled * np.float32(1e15), tiny=scaled * np.float32(1e-15))


def entries_for(shape, n, seed):
    """n descriptors: the specials, two identical entries, the 13 places (default shape) and seeded sparse matrices"""
    R, S = shape
    rng = np.random.default_rng(seed)
    out = list(special_entries(R, S).values())
    if shape == (20, 60):
        out += list(place_descriptors()[0])
    while len(out) < n:
        out.append(sparse(rng, R, S, rng.choice([0.05, 0.3, 0.8])))
    out = out[:n]
    if n > 3:
        out[-1] = out[1].copy()                                              # two identical entries
    return np.stack(out)


def fill_bank(pkg, ndt, entries, ids):
    pkg.scanContextBankClear(ndt)
    for i, e in zip(ids, entries):
        pkg.scanContextBankPut(ndt, int(i), e)
    assert pkg.scanContextBankCount(ndt) == len(set(int(i) for i in ids))


def assert_match(pkg, ndt, query, entries_sorted, ids_sorted, what):
    got = pkg.scanContextMatch(ndt, query)
    d, s, c = scan_context_match_numpy(query, entries_sorted)
    assert got["ids"].tolist() == [int(i) for i in ids_sorted], what
    assert same_bits(got["distance"].view(np.uint64), d.view(np.uint64)), (what, np.nonzero(got["distance"] != d)[0][:5])
    assert same_bits(got["shift"], s) and same_bits(got["columns"], c), what
    return got


@pytest.mark.parametrize("shape,sizes", [((20, 60), (1, 2, 65, 300)), ((1, 3), (1, 65)), ((32, 128), (2, 65)), ((20, 64), (65,)),
                                         ((20, 65), (65,))], ids=["20x60", "1x3", "32x128", "20x64", "20x65"])
def test_match_bits_equal_the_restatement(pkg, shape, sizes):
    R, S = shape
    ndt = engine(pkg)
    pkg.setScanContextParams(ndt, n_rings=R, n_sectors=S)
    sp = special_entries(R, S, seed=31)
    queries = dict(sp, random=sparse(np.random.default_rng(2), R, S, 0.4))
    if shape == (20, 60):
        queries.update(place=place_descriptors()[1][3], place1=place_descriptors()[1][1])
    for n in sizes:
        entries = entries_for(shape, n, seed=40 + n)
        ids = np.random.default_rng(n).permutation(np.arange(-5, -5 + 3 * n, 3))[:n]             # unordered, negative ones too
        fill_bank(pkg, ndt, entries, ids)
        order = np.argsort(ids)
        for name, q in queries.items():
            if n == 300 and name not in ("place", "zero", "gaps", "periodic"):
                continue
            got = assert_match(pkg, ndt, q, entries[order], ids[order], (shape, n, name))
            if name == "zero":
                assert np.all(got["distance"] == 1.0) and not got["shift"].any() and not got["columns"].any()
    # the named cases, against a bank that holds the specials of another seed first
    entries = entries_for(shape, 65, seed=5)
    names = list(special_entries(R, S))
    fill_bank(pkg, ndt, entries, range(65))
    got = pkg.scanContextMatch(ndt, sp["gaps"])
    z = names.index("zero")
    assert (got["distance"][z], got["shift"][z], got["columns"][z]) == (1.0, 0, 0)                # anything against all-zero
    assert 0 < got["columns"][names.index("gaps")] < S or S == 3
    assert got["distance"][1] == got["distance"][64] and got["shift"][1] == got["shift"][64]      # two identical entries
    per = special_entries(R, S)["periodic"]
    me = pkg.scanContextMatch(ndt, per)
    k = names.index("periodic")
    assert me["shift"][k] == 0 and abs(me["distance"][k]) < 1e-12 and me["columns"][k] == S        # a tie: the smallest shift
    period = next(q for q in (4, 5, 3, 2, 1) if S % q == 0)
    if period > 1 and R > 1:                                                 # (one ring: any two occupied columns are parallel)
        rolled = pkg.scanContextMatch(ndt, np.roll(per, -1, axis=1))                              # Q[:, j] == C[:, j + 1]
        assert rolled["shift"][k] == 1 and abs(rolled["distance"][k]) < 1e-12


def test_an_entry_keeps_its_bits_whatever_the_bank_holds(pkg):
    ndt = engine(pkg)
    entries = entries_for((20, 60), 300, seed=77)
    q = place_descriptors()[1][7]
    fill_bank(pkg, ndt, entries, range(300))
    full = pkg.scanContextMatch(ndt, q)
    assert len(full["ids"]) == 300
    for i in (0, 1, 17, 64, 299):                                            # alone
        fill_bank(pkg, ndt, entries[i:i + 1], [i])
        one = pkg.scanContextMatch(ndt, q)
        assert one["ids"].tolist() == [i]
        for k in ("distance", "shift", "columns"):
            assert same_bits(one[k], full[k][i:i + 1]), (i, k)
    # unrelated puts and erases: freed slots are reused, ids are re-ordered, the bank grows past its first allocation
    fill_bank(pkg, ndt, entries[:70], range(70))
    for i in range(0, 70, 2):
        pkg.scanContextBankErase(ndt, i)
    for i in range(70, 300):
        pkg.scanContextBankPut(ndt, 1000 - i, entries[i])                    # ids in front of nothing: 701 .. 930, descending
    for i in range(0, 70, 2):
        pkg.scanContextBankPut(ndt, i, entries[i])
    pkg.scanContextBankPut(ndt, 33, entries[33])                             # a replacement by the same descriptor
    assert pkg.scanContextBankCount(ndt) == 300
    mixed = pkg.scanContextMatch(ndt, q)
    ids = list(range(70)) + [1000 - i for i in range(299, 69, -1)]
    src = list(range(70)) + list(range(299, 69, -1))
    assert mixed["ids"].tolist() == ids
    for k in ("distance", "shift", "columns"):
        assert same_bits(mixed[k], full[k][src]), k
    for i in (0, 33, 69):
        assert same_bits(pkg.scanContextBankGet(ndt, i), entries[i])
    # match_keyframe = match of bank_get
    a, b = pkg.scanContextMatchKeyframe(ndt, 33), pkg.scanContextMatch(ndt, pkg.scanContextBankGet(ndt, 33))
    for k in ("ids", "distance", "shift", "columns"):
        assert same_bits(a[k], b[k]), k
    # unknown ids and a short output
    L = pkg.lib()
    assert code_of(pkg, pkg.scanContextBankGet, ndt, 5000) == INVALID_ARG
    assert code_of(pkg, pkg.scanContextBankErase, ndt, 5000) == INVALID_ARG
    assert code_of(pkg, pkg.scanContextMatchKeyframe, ndt, 5000) == INVALID_ARG
    assert code_of(pkg, pkg.scanContextKeyframe, ndt, 5000) == INVALID_ARG
    d = np.ascontiguousarray(q)
    assert L.ndt_scan_context_match(ndt._h, d.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, None, 299) == INVALID_ARG
    assert L.ndt_scan_context_match(ndt._h, d.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, None, 300) == 300   # every output may be NULL
    assert L.ndt_scan_context_match_keyframe(ndt._h, 33, None, None, None, None, 10) == INVALID_ARG
    assert pkg.scanContextBankCount(ndt) == 300


def test_saved_descriptors_rebuild_the_bank(pkg, rig):
    ndt = rig["ndt"]
    other = engine(pkg)
    ids = list(range(N_PLACES)) + list(range(100, 100 + N_PLACES))
    for i in ids:
        pkg.scanContextBankPut(other, i, pkg.scanContextBankGet(ndt, i))
    for i in (100, 106, 112):
        a, b = pkg.scanContextMatchKeyframe(ndt, i), pkg.scanContextMatchKeyframe(other, i)
        for k in ("ids", "distance", "shift", "columns"):
            assert same_bits(a[k], b[k]), k


# ---- 3. state -----------------------------------------------------------------------------------------------------------
def test_state_rules(pkg, rig):
    p = places()
    ndt = engine(pkg)
    assert pkg.scanContextBankCount(ndt) == 0
    empty = pkg.scanContextMatch(ndt, rig["query"][0])
    assert all(len(empty[k]) == 0 for k in empty)                            # an empty bank returns 0
    for i in range(3):
        ndt.putKeyframe(i, p["bank"][i])
        pkg.scanContextKeyframe(ndt, i)
    assert pkg.scanContextBankCount(ndt) == 3
    before = pkg.scanContextMatch(ndt, rig["query"][1])
    # the same parameters again: nothing happens; refused ones: nothing happens either
    pkg.setScanContextParams(ndt, **pkg.getScanContextParams(ndt))
    assert pkg.scanContextBankCount(ndt) == 3
    for bad in (dict(n_rings=0), dict(n_sectors=129), dict(max_radius=float("nan")), dict(z_sign=0.0), dict(lift=float("inf")),
                dict(min_points_per_bin=0)):
        assert code_of(pkg, lambda kw=bad: pkg.setScanContextParams(ndt, **kw)) == INVALID_ARG
    assert pkg.getScanContextParams(ndt)["n_rings"] == 20 and pkg.scanContextBankCount(ndt) == 3
    # ndt_keyframe_erase leaves the bank alone
    assert pkg.lib().ndt_keyframe_erase(ndt._h, 1) == 0
    assert pkg.scanContextBankCount(ndt) == 3 and same_bits(pkg.scanContextBankGet(ndt, 1), rig["bank"][1])
    after = pkg.scanContextMatch(ndt, rig["query"][1])
    for k in before:
        assert same_bits(before[k], after[k]), k
    assert code_of(pkg, pkg.scanContextKeyframe, ndt, 1) == INVALID_ARG      # the scan is gone; its descriptor stays
    assert pkg.scanContextBankCount(ndt) == 3
    # a change clears the bank: every parameter counts
    for change in (dict(n_rings=19), dict(n_sectors=61), dict(max_radius=79.0), dict(z_sign=-1.0), dict(lift=2.5), dict(min_points_per_bin=2)):
        pkg.scanContextBankPut(ndt, 5, np.zeros((pkg.getScanContextParams(ndt)["n_rings"], pkg.getScanContextParams(ndt)["n_sectors"]), np.float32))
        assert pkg.scanContextBankCount(ndt) >= 1
        pkg.setScanContextParams(ndt, **change)
        assert pkg.scanContextBankCount(ndt) == 0, change
    assert pkg.getScanContextParams(ndt) == dict(n_rings=19, n_sectors=61, max_radius=79.0, z_sign=-1.0, lift=2.5, min_points_per_bin=2)
    d = pkg.scanContextKeyframe(ndt, 0)                                      # larger descriptors than the bank was sized for
    assert d.shape == (19, 61) and pkg.scanContextBankCount(ndt) == 1
    want = scan_context_numpy(p["bank"][0], pkg.scanContextSectorTable(61), **pkg.getScanContextParams(ndt))[0]
    assert same_bits(d, want)


def test_an_align_is_left_alone(pkg, rig):
    cfg = pkg.synth.config_c1(max_points=6000)
    ndt = engine(pkg, step_size=0.1, trans_epsilon=1e-4, max_iterations=50)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    T0 = ndt.align(cfg["guess"])
    r0 = ndt.getResult()
    p = places()
    ndt.putKeyframe(3, p["bank"][3])
    d = pkg.scanContextKeyframe(ndt, 3)
    q = pkg.scanContext(ndt, p["query"][3])
    pkg.scanContextBankPut(ndt, 4, rig["bank"][4])
    m = pkg.scanContextMatch(ndt, q)
    assert same_bits(d, rig["bank"][3]) and same_bits(q, rig["query"][3]) and int(np.argmin(m["distance"])) == 0
    pkg.scanContextMatchKeyframe(ndt, 4)
    pkg.scanContextBankErase(ndt, 4)
    T1 = ndt.align(cfg["guess"])
    r1 = ndt.getResult()
    assert same_bits(T1.view(np.uint64), T0.view(np.uint64))
    for k in ("pose", "hessian"):
        assert same_bits(np.asarray(r1[k]).view(np.uint64), np.asarray(r0[k]).view(np.uint64)), k
    assert (r1["iterations"], r1["n_evaluations"], r1["transform_probability"], r1["nvtl"]) == \
           (r0["iterations"], r0["n_evaluations"], r0["transform_probability"], r0["nvtl"])


# ---- 4. end to end: the shift closes a loop the identity guess does not ---------------------------------------------------
def test_loop_closure_end_to_end(pkg, O, rig):
    from slam_sam_amd import synth
    i = CLOSURE_QUERY
    p = places()
    ndt = engine(pkg, resolution=CLOSURE_RESOLUTION, **CLOSURE_KW)
    ndt.putKeyframe(i, p["bank"][i])
    ndt.putKeyframe(100 + i, p["query"][i])
    pkg.scanContextKeyframe(ndt, i)
    q = pkg.scanContextKeyframe(ndt, 100 + i)
    pkg.scanContextBankErase(ndt, 100 + i)
    for j in range(N_PLACES):                                                # the other places, as saved descriptors
        if j != i:
            pkg.scanContextBankPut(ndt, j, rig["bank"][j])
    m = pkg.scanContextMatch(ndt, q)
    best = int(np.argmin(m["distance"]))
    shift = int(m["shift"][best])
    assert m["ids"][best] == i and shift == p["k"][i]
    c = closure_case(pkg, O, shift)
    ndt.setInputTargetFromKeyframes([i], [np.eye(4)])
    ndt.setInputSourceFromKeyframe(100 + i)
    for name, guess, ref in (("scan context", c["guess"], c["ref_sc"]), ("identity", np.eye(4), c["ref_id"])):
        T = ndt.align(guess)
        r = ndt.getResult()
        dt, dr = synth.pose_error(T, ref["T"])
        gt, gr = synth.pose_error(T, c["truth"])
        print("%s guess: %d iterations (oracle %d), %.2e m %.2e rad from the oracle, %.4f m %.3f deg from the true pose"
              % (name, r["iterations"], ref["iterations"], dt, dr, gt, np.rad2deg(gr)))
        assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD, (name, dt, dr)
        assert r["converged"] == bool(ref["converged"])
        if name == "identity":
            assert not (gt < CLOSURE_TOL_M and gr < CLOSURE_TOL_RAD)
        else:
            assert gt < CLOSURE_TOL_M and gr < CLOSURE_TOL_RAD


# ---- 5. the C++ adapter -------------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, tmp_path):
    """tests/cpp/test_scan_context.cpp against the API mocks, built with the g++ line tests/cpp/Makefile uses for them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "tests", "cpp")
    exe = str(tmp_path / "test_scan_context")
    lib = os.path.join(root, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(root, "include", "compat"), "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(d, "test_scan_context.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "scan_context: PASS" in p.stdout
