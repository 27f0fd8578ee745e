"""CPU checks of Scan Context place recognition (ndt_scan_context*; no GPU): the fourteen symbols are declared, exported,
listed and bound with ABI version 3 unchanged; arguments are refused before the handle is looked at, and the Python mirror
refuses misshapen input before the library is called; the sector table has the properties the rule leans on; the k_sc_*
kernels compile for gfx950 without scratch.
The NumPy yardstick the GPU tests compare with lives here: `scan_context_numpy` is the descriptor rule of
include/ndt_hip.h and `scan_context_match_numpy` the match rule, operation for operation -- the sums over r and j are
explicit sequential accumulations (never np.sum, which adds pairwise); only the independent axes (points, shifts, bank
entries) are vectorised.  Its own check: on a simulated street it recognises 13 places under arbitrary headings."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_scan_context_default_params", "ndt_scan_context_set_params", "ndt_scan_context_get_params",
       "ndt_scan_context_sector_table", "ndt_scan_context", "ndt_scan_context_device", "ndt_scan_context_keyframe",
       "ndt_scan_context_bank_put", "ndt_scan_context_bank_get", "ndt_scan_context_bank_erase", "ndt_scan_context_bank_clear",
       "ndt_scan_context_bank_count", "ndt_scan_context_match", "ndt_scan_context_match_keyframe")
DEFAULTS = dict(n_rings=20, n_sectors=60, max_radius=80.0, z_sign=1.0, lift=2.0, min_points_per_bin=1)


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def sector_of(dirs, x, y):
    """the one s with c_s >= 0 and c_{s+1} < 0, c_k = (double)dir[k].x * (double)y - (double)dir[k].y * (double)x, for
    points off the origin (x, y float32 arrays)"""
    d = np.asarray(dirs, np.float32).astype(np.float64)
    xd, yd = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    c = d[None, :, 0] * yd[:, None] - d[None, :, 1] * xd[:, None]
    hit = (c >= 0.0) & (np.roll(c, -1, axis=1) < 0.0)
    assert np.all(hit.sum(axis=1) == 1), "the sector must exist and be unique"
    return np.argmax(hit, axis=1)


def scan_context_numpy(points, dirs, n_rings=20, n_sectors=60, max_radius=80.0, z_sign=1.0, lift=2.0, min_points_per_bin=1):
    """The descriptor rule: (desc [R, S] float32, count [R, S] int32) of points [n, >= 3] float32; dirs: the sector table
    as ndt_scan_context_sector_table returns it."""
    R, S = int(n_rings), int(n_sectors)
    assert np.asarray(dirs).shape == (S, 2)
    p = np.asarray(points, np.float32)
    assert p.ndim == 2 and p.shape[1] >= 3
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    max_r = float(np.float32(max_radius))
    with np.errstate(all="ignore"):
        xd, yd = x.astype(np.float64), y.astype(np.float64)
        r2 = xd * xd + yd * yd
        rho = np.sqrt(r2)
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~((x == 0) & (y == 0)) & (rho < max_r)
    x, y, z, rho = x[keep], y[keep], z[keep], rho[keep]
    desc, count = np.zeros(R * S, np.float32), np.zeros(R * S, np.int32)
    if len(x):
        ring = np.minimum((rho * float(R) / max_r).astype(np.int64), R - 1)
        s = sector_of(dirs, x, y)
        with np.errstate(over="ignore"):
            hgt = np.float32(z_sign) * z + np.float32(lift)                   # f32: an exact product, one rounding
        assert hgt.dtype == np.float32
        val = np.where(hgt > 0, hgt, np.float32(0.0)).astype(np.float32)      # max(hgt, +0)
        b = ring * S + s
        np.add.at(count, b, 1)
        np.maximum.at(desc, b, val)
    desc[count < int(min_points_per_bin)] = 0.0
    return desc.reshape(R, S), count.reshape(R, S)


def scan_context_match_numpy(Q, bank):
    """The match rule: (distance float64, shift, columns) of the query Q [R, S] against one entry [R, S] (scalars) or a
    bank [B, R, S] (arrays of B).  Sequential over r and over j; vectorised over the shifts and the entries."""
    Q = np.asarray(Q, np.float32).astype(np.float64)
    Cb = np.asarray(bank, np.float32).astype(np.float64)
    single = Cb.ndim == 2
    if single:
        Cb = Cb[None]
    B, R, S = Cb.shape
    assert Q.shape == (R, S)
    with np.errstate(all="ignore"):
        q2, c2 = np.zeros(S), np.zeros((B, S))
        for r in range(R):
            q2 = q2 + Q[r] * Q[r]
            c2 = c2 + Cb[:, r] * Cb[:, r]
        nQ, nC = np.sqrt(q2), np.sqrt(c2)
        shifts = np.arange(S)
        total, m = np.zeros((B, S)), np.zeros((B, S), np.int64)               # per entry, per shift n
        for j in range(S):
            if nQ[j] == 0.0:
                continue
            jj = (j + shifts) % S
            dot = np.zeros((B, S))
            for r in range(R):
                dot = dot + Q[r, j] * Cb[:, r, jj]
            ok = nC[:, jj] != 0.0
            term = 1.0 - dot / (nQ[j] * nC[:, jj])
            total = np.where(ok, total + term, total)
            m += ok
        d = np.where(m > 0, total / np.maximum(m, 1), 1.0)
    best, at = d[:, 0].copy(), np.zeros(B, np.int64)
    for n in range(1, S):                                                     # the smallest shift that attains the minimum
        less = d[:, n] < best
        best, at = np.where(less, d[:, n], best), np.where(less, n, at)
    cols = m[np.arange(B), at].astype(np.int32)
    if single:
        return float(best[0]), int(at[0]), int(cols[0])
    return best, at.astype(np.int32), cols


def sector_table(pkg, S):
    return pkg.scanContextSectorTable(S)


# ---- the scene ----------------------------------------------------------------------------------------------------------
N_PLACES = 13


@functools.lru_cache(maxsize=None)
def places():
    """13 places along the street of synth.Scene(seed=42), seen by a 32 x 512 lidar with a 45 degree field of view: the
    bank scans at x = -90, -75 .. 90 (yaw 0) and one query per place under heading 2 pi k / 60 and a small offset.
    dict(bank [13 clouds], query [13 clouds], k [13], bank_pose, query_pose)."""
    from slam_sam_amd import synth
    sim = synth.OusterSim(synth.Scene(seed=42), beams=32, cols=512, fov_deg=45)
    rng = np.random.default_rng(3)
    out = dict(bank=[], query=[], k=[], bank_pose=[], query_pose=[])
    for i in range(N_PLACES):
        xi = -90.0 + 15.0 * i
        Tb = synth.pose_matrix(xi, 0.0, 2.0, 0.0, 0.0, 0.0)
        out["bank"].append(sim.scan(Tb, seed=100 + i))
        k = int(rng.integers(0, 60))
        dx, dy = rng.uniform(-0.7, 0.7, 2)
        Tq = synth.pose_matrix(xi + dx, dy, 2.0, 0.01, -0.01, 2.0 * np.pi * k / 60.0)
        out["query"].append(sim.scan(Tq, seed=999 + i))
        out["k"].append(k)
        out["bank_pose"].append(Tb)
        out["query_pose"].append(Tq)
    return out


@functools.lru_cache(maxsize=None)
def place_descriptors():
    """(bank [13, 20, 60], query [13, 20, 60]) of places() under the default parameters, by the restatement"""
    import __graft_entry__ as ge
    dirs = ge.load_package().scanContextSectorTable(60)
    p = places()
    bank = np.stack([scan_context_numpy(c, dirs)[0] for c in p["bank"]])
    query = np.stack([scan_context_numpy(c, dirs)[0] for c in p["query"]])
    bank.setflags(write=False)
    query.setflags(write=False)
    return bank, query


# ---- the sector table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 4, 59, 60, 64, 65, 127, 128])
def test_sector_table(pkg, S):
    d = sector_table(pkg, S)
    assert d.dtype == np.float32 and d.shape == (S, 2)
    assert d[0, 0] == 1.0 and d[0, 1] == 0.0 and not np.signbit(d[0, 1])
    a = 2.0 * np.pi * np.arange(S) / S
    want = np.stack([np.cos(a), np.sin(a)], 1)
    w32 = want.astype(np.float32)
    ulp = np.maximum(np.spacing(np.abs(w32)), np.spacing(np.float32(0)))
    assert np.all(np.abs(d.astype(np.float64) - w32.astype(np.float64)) <= ulp)       # within 1 f32 ulp of NumPy's
    # strict angular order: every next direction is counter-clockwise of the previous (exact in f64), less than half a turn
    dd = d.astype(np.float64)
    nxt = np.roll(dd, -1, axis=0)
    assert np.all(dd[:, 0] * nxt[:, 1] - dd[:, 1] * nxt[:, 0] > 0)
    ang = np.unwrap(np.arctan2(dd[:, 1], dd[:, 0]))
    assert np.all(np.diff(ang) > 0) and ang[-1] - ang[0] < 2 * np.pi
    # a point on a table direction belongs to that sector or, by the rounding of dir, to the one before: nowhere else
    s = sector_of(d, d[:, 0] * np.float32(7.0), d[:, 1] * np.float32(7.0))
    assert np.all((s == np.arange(S)) | (s == (np.arange(S) - 1) % S))
    L = pkg.lib()
    buf = (C.c_float * 256)()
    assert L.ndt_scan_context_sector_table(2, buf) == -1 and L.ndt_scan_context_sector_table(129, buf) == -1
    assert L.ndt_scan_context_sector_table(60, None) == -1 and not any(buf)


# ---- the restatement's own checks ---------------------------------------------------------------------------------------
def test_restatement_by_hand(pkg):
    d4 = sector_table(pkg, 4)
    pts = np.array([[1, 0.5, 1], [1, 0.5, 3], [-1, 0.5, -5], [0, 0, 9], [np.nan, 1, 1], [3.9, -0.1, 0.5], [1, 1, np.inf]], np.float32)
    desc, count = scan_context_numpy(pts, d4, n_rings=2, n_sectors=4, max_radius=4.0, z_sign=1.0, lift=2.0)
    assert count.tolist() == [[2, 1, 0, 0], [0, 0, 0, 1]] and count.dtype == np.int32 and desc.dtype == np.float32
    assert desc[0, 0] == 5.0 and desc[0, 1] == 0.0 and desc[1, 3] == 2.5 and not np.signbit(desc).any()
    desc3, _ = scan_context_numpy(pts, d4, n_rings=2, n_sectors=4, max_radius=4.0, min_points_per_bin=2)
    assert desc3[0, 0] == 5.0 and desc3[1, 3] == 0.0
    down, _ = scan_context_numpy(pts, d4, n_rings=2, n_sectors=4, max_radius=4.0, z_sign=-1.0, lift=2.0)
    assert down[0, 0] == 1.0 and down[0, 1] == 7.0
    # the match: a descriptor against itself rolled by 3 columns -> distance ~0 at shift 3; empty against anything -> 1, 0, 0
    rng = np.random.default_rng(0)
    Q = (rng.random((5, 12)) * (rng.random((5, 12)) < 0.6)).astype(np.float32)
    Cm = np.roll(Q, 3, axis=1)                                                        # Q[:, j] == C[:, j + 3]
    dist, shift, cols = scan_context_match_numpy(Q, Cm)
    assert shift == 3 and abs(dist) < 1e-15 and cols == int((np.linalg.norm(Q, axis=0) > 0).sum())
    assert scan_context_match_numpy(np.zeros((5, 12)), Cm) == (1.0, 0, 0)
    assert scan_context_match_numpy(Q, np.zeros((5, 12))) == (1.0, 0, 0)
    per = np.tile(Q[:, :4], (1, 3))                                                   # periodic in 4 sectors: a tie, smallest shift
    assert scan_context_match_numpy(per, per)[1] == 0
    assert scan_context_match_numpy(per, np.roll(per, 1, axis=1))[1] == 1
    batch = scan_context_match_numpy(Q, np.stack([Cm, np.zeros((5, 12), np.float32), Q]))
    assert batch[1].tolist() == [3, 0, 0] and batch[0][1] == 1.0 and batch[2][1] == 0
    assert batch[0][0].tobytes() == np.float64(dist).tobytes()                        # an entry alone = the entry in a bank


def test_the_rule_recognises_places():
    """Default parameters, 13 places, 13 queries under arbitrary headings: every query's best entry is its own place, every
    shift is k or k + 30 (the street's 180 degree symmetry; query 1), at least 12 are k."""
    p = places()
    bank, query = place_descriptors()
    n_exact = 0
    for i in range(N_PLACES):
        dist, shift, cols = scan_context_match_numpy(query[i], bank)
        best = int(np.argmin(dist))
        wrong = np.delete(dist, i).min()
        k = p["k"][i]
        print("query %2d: best place %2d, distance %.3f (best wrong place %.3f), shift %2d (k = %2d), %d columns"
              % (i, best, dist[i], wrong, shift[i], k, cols[i]))
        assert best == i
        assert shift[i] in (k, (k + 30) % 60)
        n_exact += int(shift[i] == k)
    assert n_exact >= 12


# ---- the loop closure the GPU test closes end to end ----------------------------------------------------------------------
# Chosen on the CPU oracle among the 13 queries and resolutions 1, 2 and 3 m: query 4 (k = 27, 162 degrees) at 2.0 m.
CLOSURE_QUERY, CLOSURE_RESOLUTION = 4, 2.0
CLOSURE_KW = dict(step_size=0.1, trans_epsilon=1e-4, max_iterations=50)
CLOSURE_TOL_M, CLOSURE_TOL_RAD = 0.3, np.deg2rad(2.0)


def closure_case(pkg, O, shift):
    """The oracle's aligns of query scan 4 (source) to place 4's scan (target) from Rz(scanContextYaw(shift)) and from the
    identity: dict(truth, guess, ref_sc, ref_id)"""
    from slam_sam_amd import synth
    p = places()
    i = CLOSURE_QUERY
    truth = np.linalg.inv(p["bank_pose"][i]) @ p["query_pose"][i]
    guess = synth.pose_matrix(0, 0, 0, 0, 0, pkg.scanContextYaw(shift, 60))
    grid = O.Grid(p["bank"][i], O.default_params(resolution=CLOSURE_RESOLUTION, **CLOSURE_KW))
    return dict(truth=truth, guess=guess, ref_sc=grid.align(p["query"][i], guess), ref_id=grid.align(p["query"][i], np.eye(4)))


def test_the_loop_closure_case_on_the_oracle(pkg, O):
    """From the Scan Context guess the oracle ends 0.004 m and 0.00 degrees from the true relative pose in 5 iterations;
    from the identity guess it ends 0.535 m and 180 degrees away."""
    from slam_sam_amd import synth
    bank, query = place_descriptors()
    dist, shift, _ = scan_context_match_numpy(query[CLOSURE_QUERY], bank)
    assert int(np.argmin(dist)) == CLOSURE_QUERY and shift[CLOSURE_QUERY] == places()["k"][CLOSURE_QUERY] == 27
    c = closure_case(pkg, O, int(shift[CLOSURE_QUERY]))
    dt, dr = synth.pose_error(c["ref_sc"]["T"], c["truth"])
    it, ir = synth.pose_error(c["ref_id"]["T"], c["truth"])
    print("oracle from the Scan Context guess: %.4f m %.3f deg; from identity: %.4f m %.3f deg" % (dt, np.rad2deg(dr), it, np.rad2deg(ir)))
    assert c["ref_sc"]["converged"] and dt < CLOSURE_TOL_M and dr < CLOSURE_TOL_RAD
    assert not (it < CLOSURE_TOL_M and ir < CLOSURE_TOL_RAD)


# ---- the boundary -------------------------------------------------------------------------------------------------------
DECLS = (
    "typedef struct { int32_t n_rings, n_sectors; float max_radius, z_sign, lift; int32_t min_points_per_bin; } ndt_scan_context_params;",
    "void ndt_scan_context_default_params(ndt_scan_context_params* p);",
    "int ndt_scan_context_set_params(ndt_handle* h, const ndt_scan_context_params* p);",
    "int ndt_scan_context_get_params(const ndt_handle* h, ndt_scan_context_params* p);",
    "int ndt_scan_context_sector_table(int n_sectors, float* dir_xy);",
    "int ndt_scan_context(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, float* desc, int32_t* count_or_null);",
    "int ndt_scan_context_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n, float* d_desc, int32_t* d_count_or_null);",
    "int ndt_scan_context_keyframe(ndt_handle* h, int64_t id, float* desc_or_null, int32_t* count_or_null);",
    "int ndt_scan_context_bank_put(ndt_handle* h, int64_t id, const float* desc);",
    "int ndt_scan_context_bank_get(ndt_handle* h, int64_t id, float* desc);",
    "int ndt_scan_context_bank_erase(ndt_handle* h, int64_t id);",
    "int ndt_scan_context_bank_clear(ndt_handle* h);",
    "int64_t ndt_scan_context_bank_count(const ndt_handle* h);",
    "int64_t ndt_scan_context_match(ndt_handle* h, const float* desc, int64_t* ids, double* distance, int32_t* shift, int32_t* columns, size_t cap);",
    "int64_t ndt_scan_context_match_keyframe(ndt_handle* h, int64_t id, int64_t* ids, double* distance, int32_t* shift, int32_t* columns, size_t cap);",
)


def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, dp, fp, i64 = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_int64
    scp = C.POINTER(pkg.ScanContextParams)
    want = {
        "ndt_scan_context_default_params": [scp],
        "ndt_scan_context_set_params": [vp, scp],
        "ndt_scan_context_get_params": [vp, scp],
        "ndt_scan_context_sector_table": [C.c_int, fp],
        "ndt_scan_context": [vp, vp, C.c_size_t, C.c_size_t, fp, vp],
        "ndt_scan_context_device": [vp, vp, vp, vp, C.c_size_t, vp, vp],
        "ndt_scan_context_keyframe": [vp, i64, fp, vp],
        "ndt_scan_context_bank_put": [vp, i64, fp],
        "ndt_scan_context_bank_get": [vp, i64, fp],
        "ndt_scan_context_bank_erase": [vp, i64],
        "ndt_scan_context_bank_clear": [vp],
        "ndt_scan_context_bank_count": [vp],
        "ndt_scan_context_match": [vp, fp, vp, dp, vp, vp, C.c_size_t],
        "ndt_scan_context_match_keyframe": [vp, i64, vp, dp, vp, vp, C.c_size_t],
    }
    assert set(want) == set(NEW)
    for name in NEW:
        assert re.search(r"\b(?:int|int64_t|void)\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    for name in ("ndt_scan_context_bank_count", "ndt_scan_context_match", "ndt_scan_context_match_keyframe"):
        assert getattr(L, name).restype is C.c_int64
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for decl in DECLS:
        assert decl in flat, decl
    assert C.sizeof(pkg.ScanContextParams) == 24
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    p = pkg.scanContextDefaultParams()
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    hpp = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    for m in ("setScanContextParams", "scanContext", "scanContextDevice", "scanContextKeyframe", "scanContextBankPut",
              "scanContextBankGet", "scanContextBankErase", "scanContextBankClear", "scanContextBankCount", "scanContextMatch",
              "scanContextMatchKeyframe", "scanContextYaw"):
        assert re.search(r"\b%s\s*\(" % m, hpp), m
        assert callable(getattr(pkg, m)), m
        assert not hasattr(pkg.NormalDistributionsTransform, m), m                    # functions of the package, not methods
    mk = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "Makefile")).read()
    assert "$(B)/ndt_scan_context.o" in mk and "-ffp-contract=off" in mk


def test_scan_context_yaw(pkg):
    assert pkg.scanContextYaw(0, 60) == 0.0
    assert pkg.scanContextYaw(15, 60) == pytest.approx(np.pi / 2)
    assert pkg.scanContextYaw(30, 60) == pytest.approx(np.pi) and pkg.scanContextYaw(30, 60) > 0     # (-pi, pi]
    assert pkg.scanContextYaw(31, 60) == pytest.approx(-29 * 2 * np.pi / 60)
    assert pkg.scanContextYaw(59, 60) == pytest.approx(-2 * np.pi / 60)
    assert pkg.scanContextYaw(32, 65) == pytest.approx(32 * 2 * np.pi / 65) and pkg.scanContextYaw(33, 65) < 0
    for bad in ((60, 60), (-1, 60), (0, 2)):
        with pytest.raises(ValueError):
            pkg.scanContextYaw(*bad)


def test_argument_errors_come_before_the_handle(pkg):
    L = pkg.lib()
    good = pkg.scanContextDefaultParams()
    xyz = (C.c_float * 15)(*([1.0] * 15))
    desc = (C.c_float * 4096)()
    ids = (C.c_int64 * 4)()
    out = pkg.ScanContextParams()
    dev = 4096                                                                        # a stand-in device address, never read
    # NULL handle
    assert L.ndt_scan_context_set_params(None, C.byref(good)) == -1
    assert L.ndt_scan_context_get_params(None, C.byref(out)) == -1 and out.n_rings == 0
    assert L.ndt_scan_context(None, xyz, 5, 12, desc, None) == -1
    assert L.ndt_scan_context_device(None, dev, dev, dev, 5, dev, None) == -1
    assert L.ndt_scan_context_keyframe(None, 0, desc, None) == -1
    assert L.ndt_scan_context_bank_put(None, 0, desc) == -1
    assert L.ndt_scan_context_bank_get(None, 0, desc) == -1
    assert L.ndt_scan_context_bank_erase(None, 0) == -1
    assert L.ndt_scan_context_bank_clear(None) == -1
    assert L.ndt_scan_context_bank_count(None) == -1
    assert L.ndt_scan_context_match(None, desc, ids, None, None, None, 4) == -1
    assert L.ndt_scan_context_match_keyframe(None, 0, ids, None, None, None, 4) == -1
    L.ndt_scan_context_default_params(None)                                           # nothing to fill: a no-op
    # the argument checks come before the handle is looked at: a stand-in block of zero bytes is never read or written
    h = C.create_string_buffer(1 << 16)
    assert L.ndt_scan_context_set_params(h, None) == -1
    bad = [dict(n_rings=0), dict(n_rings=33), dict(n_sectors=2), dict(n_sectors=129), dict(max_radius=0.0),
           dict(max_radius=-1.0), dict(max_radius=np.inf), dict(max_radius=np.nan), dict(z_sign=0.0), dict(z_sign=0.5),
           dict(z_sign=-2.0), dict(z_sign=np.nan), dict(lift=np.inf), dict(lift=np.nan), dict(min_points_per_bin=0),
           dict(min_points_per_bin=-3)]
    for kw in bad:
        p = pkg.scanContextDefaultParams()
        for k, v in kw.items():
            setattr(p, k, v)
        assert L.ndt_scan_context_set_params(h, C.byref(p)) == -1, kw
    assert L.ndt_scan_context_get_params(h, None) == -1
    assert L.ndt_scan_context(h, None, 5, 12, desc, None) == -1
    assert L.ndt_scan_context(h, xyz, 5, 12, None, None) == -1
    assert L.ndt_scan_context(h, xyz, 5, 8, desc, None) == -1
    assert L.ndt_scan_context(h, xyz, 5, 14, desc, None) == -1
    assert L.ndt_scan_context_device(h, None, dev, dev, 5, dev, None) == -1
    assert L.ndt_scan_context_device(h, dev, None, dev, 5, dev, None) == -1
    assert L.ndt_scan_context_device(h, dev, dev, None, 5, dev, None) == -1
    assert L.ndt_scan_context_device(h, dev, dev, dev, 5, None, None) == -1
    assert L.ndt_scan_context_bank_put(h, 0, None) == -1
    assert L.ndt_scan_context_bank_get(h, 0, None) == -1
    assert L.ndt_scan_context_match(h, None, ids, None, None, None, 4) == -1
    assert bytes(h.raw) == bytes(1 << 16) and not any(desc) and not any(ids)          # nothing was written


def test_python_mirror_validates_before_the_library(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)   # no handle: nothing may reach the library
    ndt._h = None
    bad = [
        lambda: pkg.scanContext(ndt, np.zeros(7)),
        lambda: pkg.scanContext(ndt, np.zeros((5, 2))),
        lambda: pkg.scanContext(ndt, np.zeros((2, 5, 3))),
        lambda: pkg.scanContextDevice(ndt, 0, 16, 16, 4, 16),
        lambda: pkg.scanContextDevice(ndt, 16, 16, None, 4, 16),
        lambda: pkg.scanContextDevice(ndt, 16, 16, 16, 4, None),
        lambda: pkg.scanContextDevice(ndt, 16, 16, 16, -1, 16),
        lambda: pkg.scanContextKeyframe(ndt, 1.5),
        lambda: pkg.scanContextBankPut(ndt, 0, np.zeros(1200)),
        lambda: pkg.scanContextBankPut(ndt, 0, np.zeros((2, 20, 60))),
        lambda: pkg.scanContextBankPut(ndt, 0, np.zeros((20, 60), dtype=complex)),
        lambda: pkg.scanContextBankPut(ndt, 0.5, np.zeros((20, 60))),
        lambda: pkg.scanContextBankGet(ndt, "a"),
        lambda: pkg.scanContextBankErase(ndt, 2.5),
        lambda: pkg.scanContextMatch(ndt, np.zeros(1200)),
        lambda: pkg.scanContextMatch(ndt, [["a"] * 60] * 20),
        lambda: pkg.scanContextMatchKeyframe(ndt, 0.25),
        lambda: pkg.setScanContextParams(ndt, rings=3),
        lambda: pkg.setScanContextParams(ndt, n_rings=2.5),
        lambda: pkg.scanContextSectorTable(2),
        lambda: pkg.scanContextSectorTable(60.5),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d reached the library" % k)


# ---- the kernels --------------------------------------------------------------------------------------------------------
def test_scan_context_kernels_do_not_spill(tmp_path):
    """The -Rpass-analysis=kernel-resource-usage figures of ndt_scan_context.hip under the engine's flags: three kernels,
    all k_sc_*, none with scratch."""
    path = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_scan_context.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", ln)
        if m and name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    assert usage and all("k_sc_" in k for k in usage), sorted(usage)
    kernels = {re.search(r"k_sc_[a-z_]+?(?=E)", k).group(0) for k in usage}
    assert kernels == {"k_sc_bins", "k_sc_finish", "k_sc_match"}, kernels
    for k, u in usage.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 128, (k, u)
    src = open(path).read()
    assert len(re.findall(r"__global__", src)) == len(kernels)
    # integer atomics only (max on the heights' bit patterns, add on the counts), no inline assembly
    assert set(re.findall(r"\batomic\w*\(", src)) == {"atomicAdd(", "atomicMax("} and not re.search(r"\basm\b", src)
    assert not re.search(r"atomic\w*\(\s*\(?\s*(float|double)", src)
