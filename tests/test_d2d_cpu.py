"""CPU checks of the distribution-to-distribution registration (ndt_set_source_distributions / _device,
ndt_source_distributions_info, ndt_export_source_distributions, ndt_eval_derivatives_d2d, ndt_align_d2d; no GPU): the
six symbols are declared, exported, listed and bound with ABI version 3 unchanged; arguments are refused before the
handle is looked at, and the Python mirror refuses misshapen input before the library is called; the kernels of
ndt_d2d.hip compile for gfx950 without scratch.
The NumPy yardstick the GPU tests compare with lives here: `d2d_numpy` is the evaluation rule of include/ndt_hip.h in f64,
formula for formula (the rule's q_a and q_ab as written there, the inverse by numpy.linalg.inv), `d2d_pairs` the
neighbour rule (the f32 classification of the f32-rounded moved mean and its six face-offset copies).  Its own checks:
gradient and Hessian against central differences, the Hessian's symmetry and conditioning on the align scene, and the
host Newton loop (ndt_newton_align) driven by it."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_set_source_distributions", "ndt_set_source_distributions_device", "ndt_source_distributions_info",
       "ndt_export_source_distributions", "ndt_eval_derivatives_d2d", "ndt_align_d2d")
KW = dict(step_size=0.1, trans_epsilon=1e-4, max_iterations=35)
ATTITUDE = (0.7, -0.5, 2.0)
# probe order of the DIRECT7 neighbourhood (k_point_scores): the point, then +leaf / -leaf along x, y, z
PROBES = ((0, 0.0), (0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0), (2, 1.0), (2, -1.0))


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def rot_derivs(pose6):
    """R = Rx(roll) Ry(pitch) Rz(yaw), dR[c] and d2R[c][d] (c, d over roll, pitch, yaw) from exact sin / cos in f64"""
    def axis(a, k, which):
        c, s = np.cos(a), np.sin(a)
        cc, ss = ((c, s), (-s, c), (-c, -s))[k]
        one = 1.0 if k == 0 else 0.0
        return np.array({"x": [[one, 0, 0], [0, cc, -ss], [0, ss, cc]],
                         "y": [[cc, 0, ss], [0, one, 0], [-ss, 0, cc]],
                         "z": [[cc, -ss, 0], [ss, cc, 0], [0, 0, one]]}[which], np.float64)

    def prod(o):
        return axis(pose6[3], o[0], "x") @ axis(pose6[4], o[1], "y") @ axis(pose6[5], o[2], "z")

    unit = np.eye(3, dtype=int)
    R = prod((0, 0, 0))
    dR = [prod(tuple(unit[c])) for c in range(3)]
    d2R = [[prod(tuple(unit[c] + unit[d])) for d in range(3)] for c in range(3)]
    return R, dR, d2R


def moved_means(pose6, mean):
    """m_a = ((R_a0 mu_0 + R_a1 mu_1) + R_a2 mu_2) + t_a, every operation one f64 rounding"""
    R = rot_derivs(pose6)[0]
    mu = np.asarray(mean, np.float64)
    return np.stack([((R[a, 0] * mu[:, 0] + R[a, 1] * mu[:, 1]) + R[a, 2] * mu[:, 2]) + pose6[a] for a in range(3)], axis=1)


def classify(pts32, grid):
    """the engine's f32 classification of points into the dense grid: linear cell index, -1 outside"""
    leaf = np.float32(grid["leaf_size"])
    inv = np.float32(1.0) / leaf
    min_b, max_b, div_b = (np.asarray(grid[k], np.int64) for k in ("min_b", "max_b", "div_b"))
    lo, hi = min_b.astype(np.float32) * leaf, (max_b + 1).astype(np.float32) * leaf
    p = np.asarray(pts32, np.float32)
    with np.errstate(all="ignore"):
        inside = np.isfinite(p).all(axis=1) & ((p >= lo) & (p < hi)).all(axis=1)
        f = np.floor(p * inv) - min_b.astype(np.float32)
    i = np.where(inside[:, None], f, 0).astype(np.int64)
    idx = i[:, 0] + i[:, 1] * div_b[0] + i[:, 2] * div_b[0] * div_b[1]
    ok = inside & (idx >= 0) & (idx < int(np.prod(div_b)))
    return np.where(ok, idx, -1)


def d2d_pairs(m, tgt, grid, method="DIRECT7"):
    """(source index, target leaf index) of every pair, source-major and in probe order, for moved means m [n, 3]"""
    m32 = np.asarray(m, np.float64).astype(np.float32)
    finite = np.isfinite(m32).all(axis=1)
    leaf = np.float32(grid["leaf_size"])
    cells = np.asarray(tgt["cell"], np.int64)
    assert np.all(np.diff(cells) > 0)
    pi, ps, pk = [], [], []
    for k, (axis, sign) in enumerate(PROBES[:7 if method == "DIRECT7" else 1]):
        p = m32.copy()
        if sign:
            p[:, axis] = m32[:, axis] + np.float32(sign) * leaf               # f32 add
        cell = classify(p, grid)
        at = np.clip(np.searchsorted(cells, cell), 0, max(len(cells) - 1, 0))
        hit = finite & (cell >= 0) & (len(cells) > 0) & (cells[at] == cell)
        pi.append(np.nonzero(hit)[0]); ps.append(at[hit]); pk.append(np.full(int(hit.sum()), k))
    pi, ps, pk = np.concatenate(pi), np.concatenate(ps), np.concatenate(pk)
    order = np.lexsort((pk, pi))
    return pi[order], ps[order]


def d2d_numpy(pose6, src, tgt, grid, d1, d2, method="DIRECT7", hessian=True, pairs=None):
    """The evaluation rule: dict(score, gradient [6], hessian [6, 6], nvtl_sum, n_with_neighbors, n_pairs).
    src: dict(mean [n, 3], cov [n, 3, 3]); tgt: dict(cell [L] ascending, mean, cov) -- getLeaves();
    grid: dict(min_b, max_b, div_b, leaf_size) -- getGridInfo().  pairs: a fixed pair list (central differences)."""
    pose6 = np.asarray(pose6, np.float64)
    R, dR, d2R = rot_derivs(pose6)
    mu_i, S = np.asarray(src["mean"], np.float64), np.asarray(src["cov"], np.float64)
    n = len(mu_i)
    m = moved_means(pose6, mu_i)
    pi, ps = d2d_pairs(m, tgt, grid, method) if pairs is None else pairs
    out = dict(score=0.0, gradient=np.zeros(6), hessian=np.zeros((6, 6)), nvtl_sum=0.0, n_with_neighbors=0, n_pairs=0)
    if len(pi) == 0:
        return out
    mu = m[pi] - np.asarray(tgt["mean"], np.float64)[ps]
    A = np.einsum("ab,nbc,dc->nad", R, S, R)
    B = np.linalg.inv(A[pi] + np.asarray(tgt["cov"], np.float64)[ps])
    v = np.einsum("pab,pb->pa", B, mu)
    with np.errstate(all="ignore"):
        e = np.exp(-d2 * np.einsum("pa,pa->p", mu, v) / 2.0)
    ok = np.isfinite(e) & (e >= 0.0) & (e <= 1.0)                          # the evaluation's guard
    pi, B, v, e = pi[ok], B[ok], v[ok], e[ok]
    P = len(pi)
    sc = -d1 * e
    best = np.zeros(n)
    np.maximum.at(best, pi, sc)
    out.update(score=float(sc.sum()), nvtl_sum=float(best.sum()), n_with_neighbors=len(np.unique(pi)), n_pairs=P)
    j = np.zeros((P, 6, 3))
    Z = np.zeros((P, 6, 3, 3))
    j[:, :3] = np.eye(3)
    for c in range(3):
        j[:, 3 + c] = (mu_i @ dR[c].T)[pi]
        M = np.einsum("ab,nbc,dc->nad", dR[c], S, R)
        Z[:, 3 + c] = (M + M.transpose(0, 2, 1))[pi]
    Bj = np.einsum("pab,pkb->pka", B, j)
    Zv = np.einsum("pkab,pb->pka", Z, v)
    qa = 2.0 * np.einsum("pa,pka->pk", v, j) - np.einsum("pa,pka->pk", v, Zv)
    f = (d1 * d2 / 2.0) * e
    out["gradient"] = (f[:, None] * qa).sum(axis=0)
    if not hessian:
        return out
    BZv = np.einsum("pab,pkb->pka", B, Zv)
    qab = (2.0 * np.einsum("pbx,pax->pab", j, Bj) - 2.0 * np.einsum("pbx,pax->pab", Zv, Bj)
           - 2.0 * np.einsum("pbx,pax->pab", j, BZv) + 2.0 * np.einsum("pbx,pax->pab", Zv, BZv))
    for c in range(3):
        for d in range(3):
            Hcd = (mu_i @ d2R[c][d].T)[pi]
            N = np.einsum("ab,nbc,dc->nad", d2R[c][d], S, R) + np.einsum("ab,nbc,dc->nad", dR[c], S, dR[d])
            Zcd = (N + N.transpose(0, 2, 1))[pi]
            qab[:, 3 + c, 3 + d] += 2.0 * np.einsum("pa,pa->p", v, Hcd) - np.einsum("pa,pab,pb->p", v, Zcd, v)
    out["hessian"] = (f[:, None, None] * (qab - (d2 / 2.0) * qa[:, :, None] * qa[:, None, :])).sum(axis=0)
    return out


def gauss_constants(pkg, resolution=1.0, outlier_ratio=0.55):
    a, b = C.c_double(), C.c_double()
    fn = pkg.lib().ndt_gauss_constants
    fn.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    assert fn(resolution, outlier_ratio, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


# ---- the scene ----------------------------------------------------------------------------------------------------------
TRUE_POSE6 = (0.25, -0.15, 0.08, np.deg2rad(0.8), np.deg2rad(-0.6), np.deg2rad(1.7))      # about 0.3 m and 2 degrees


@functools.lru_cache(maxsize=None)
def scene(seed=11):
    """Hilly ground and the vertical faces of ten buildings on 48 m x 48 m (synth's wide surfaces): all six degrees of
    freedom are held.  target: 36 000 points; source: 30 000 points of ANOTHER sample of the same surfaces, moved by the
    inverse of `truth` (the pose an align has to find).  Both float32 [n, 3]."""
    from slam_sam_amd import synth
    rng = np.random.default_rng(seed)
    half = 24.0
    boxes = np.stack([rng.uniform(-half + 5, half - 5, 10), rng.uniform(-half + 5, half - 5, 10), rng.uniform(2.0, 5.0, 10),
                      rng.uniform(2.0, 5.0, 10), rng.uniform(4.0, 8.0, 10)], 1)
    tgt = synth._wide_surfaces(rng, 24000, 12000, half, boxes)
    tgt = (tgt + rng.normal(0.0, 0.02, tgt.shape)).astype(np.float32)
    rs = np.random.default_rng(seed + 1)
    world = synth._wide_surfaces(rs, 20000, 10000, half - 2.0, boxes)
    world = world + rs.normal(0.0, 0.02, world.shape)
    truth = synth.pose_matrix(*TRUE_POSE6)
    src = synth.transform(np.linalg.inv(truth), world).astype(np.float32)
    return dict(target=tgt, source=src, truth=truth)


def oracle_side(O, cloud):
    prm = O.default_params(resolution=1.0, num_threads=8, **KW)
    g = O.Grid(cloud, prm)
    return g.export(), dict(min_b=g.min_b, max_b=g.max_b, div_b=g.div_b, leaf_size=1.0)


@pytest.fixture(scope="module")
def sides(O):
    s = scene()
    tgt, grid = oracle_side(O, s["target"])
    src, _ = oracle_side(O, s["source"])
    assert 2000 < len(src["mean"]) < 6000 and 2000 < len(tgt["mean"]) < 6000
    return dict(src=src, tgt=tgt, grid=grid, truth=s["truth"])


def restatement_evaluator(pkg, src, tgt, grid, d1, d2, method="DIRECT7", log=None):
    def ev(pose6, T, need_h):
        r = d2d_numpy(pose6, src, tgt, grid, d1, d2, method, hessian=bool(need_h))
        if log is not None:
            log.append(np.array(pose6))
        return pkg.pack_eval(r["score"], r["gradient"], r["hessian"], r["nvtl_sum"], r["n_with_neighbors"], r["n_pairs"])
    return ev


# ---- the yardstick's own checks -----------------------------------------------------------------------------------------
# Central differences of an f64 function with step h carry a truncation error of h^2 / 6 times the third derivative and a
# rounding error of about eps |f| / h.  Here f is the score (or a gradient component): a sum of ~2e4 terms of size |d1|
# ~ 1, so |f| <~ 1e4 and eps |f| / h = 1e-7 at h = 1e-5, against gradient components of 1e2 .. 1e4: <~ 1e-9 of the norm.
# Each pair's exponent is -d2 q / 2 with q quadratic in the pose; per derivative the terms grow by at most the lever arm
# times d2 |B mu| ~ 35 m x 10, so third / first derivative <~ 1e5 and h^2 / 6 of that is ~ 2e-6 at worst, typically far
# less since the terms do not add coherently.  h = 1e-5 balances the two; the bound is 1e-5 of the norm.
FD_STEP, FD_TOL = 1e-5, 1e-5


@pytest.mark.parametrize("attitude", [(0.0, 0.0, 0.0), ATTITUDE], ids=["identity", "attitude"])
@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT1"])
def test_gradient_and_hessian_are_the_central_differences(pkg, sides, attitude, method):
    d1, d2 = gauss_constants(pkg)
    src, tgt, grid = sides["src"], sides["tgt"], sides["grid"]
    pose = np.array([0.21, -0.13, 0.05, *attitude])
    if any(attitude):
        # far from the identity the source is put where the rotated cloud overlaps the target: rotate it back first
        from slam_sam_amd import synth
        back = np.linalg.inv(synth.pose_matrix(0, 0, 0, *attitude))[:3, :3]
        src = dict(mean=src["mean"] @ back.T, cov=np.einsum("ab,nbc,dc->nad", back, src["cov"], back))
    pairs = d2d_pairs(moved_means(pose, src["mean"]), tgt, grid, method)
    assert len(pairs[0]) > (5000 if method == "DIRECT7" else 1500)
    at = d2d_numpy(pose, src, tgt, grid, d1, d2, method, pairs=pairs)
    assert at["n_pairs"] > 0.9 * len(pairs[0]) and at["score"] > 0
    assert np.array_equal(at["hessian"], at["hessian"].T) or np.abs(at["hessian"] - at["hessian"].T).max() <= 1e-12 * np.abs(at["hessian"]).max()
    g_fd, H_fd = np.zeros(6), np.zeros((6, 6))
    for a in range(6):
        hi, lo = pose.copy(), pose.copy()
        hi[a] += FD_STEP
        lo[a] -= FD_STEP
        rh = d2d_numpy(hi, src, tgt, grid, d1, d2, method, hessian=False, pairs=pairs)
        rl = d2d_numpy(lo, src, tgt, grid, d1, d2, method, hessian=False, pairs=pairs)
        assert rh["n_pairs"] == rl["n_pairs"] == at["n_pairs"]                # the guard cuts the same pairs
        g_fd[a] = (rh["score"] - rl["score"]) / (2 * FD_STEP)
        H_fd[a] = (rh["gradient"] - rl["gradient"]) / (2 * FD_STEP)
    eg = np.linalg.norm(at["gradient"] - g_fd) / np.linalg.norm(at["gradient"])
    eh = np.linalg.norm(at["hessian"] - H_fd) / np.linalg.norm(at["hessian"])
    print("central differences %s %s: gradient %.2e, Hessian %.2e of their norms" % (method, attitude, eg, eh))
    assert eg < FD_TOL and eh < FD_TOL, (eg, eh)
    # without the Hessian the score and the gradient are the same numbers
    no_h = d2d_numpy(pose, src, tgt, grid, d1, d2, method, hessian=False, pairs=pairs)
    assert no_h["score"] == at["score"] and np.array_equal(no_h["gradient"], at["gradient"]) and not no_h["hessian"].any()


def test_the_scene_holds_all_six_degrees_of_freedom(pkg, sides):
    d1, d2 = gauss_constants(pkg)
    from slam_sam_amd import synth
    r = d2d_numpy(np.array(TRUE_POSE6), sides["src"], sides["tgt"], sides["grid"], d1, d2)
    w = np.linalg.eigvalsh(-r["hessian"])
    print("eigenvalues of -H at the true pose: %s" % w)
    assert w.min() > 0 and w.max() / w.min() < 1e5, w                         # a maximum, and no direction is loose
    assert r["n_with_neighbors"] > 0.8 * len(sides["src"]["mean"])
    assert np.allclose(synth.pose_matrix(*TRUE_POSE6), sides["truth"])


def test_newton_align_over_the_restatement_converges(pkg, sides):
    """ndt_newton_align driven by d2d_numpy from the identity guess on the align scene: converged after 10 iterations
    (13 evaluations), 0.0037 m and 1.19e-4 rad from the true pose (the two samples of the surfaces differ; the voxel
    statistics of 1 m leaves carry that much)."""
    from slam_sam_amd import synth
    d1, d2 = gauss_constants(pkg)
    log = []
    ev = restatement_evaluator(pkg, sides["src"], sides["tgt"], sides["grid"], d1, d2, log=log)
    r = pkg.newton_align(pkg.default_params(resolution=1.0, **KW), len(sides["src"]["mean"]), np.eye(4), ev)
    dt, dr = synth.pose_error(r["T"], sides["truth"])
    print("newton_align over the restatement: %d iterations, %d evaluations, %.4f m %.2e rad from the true pose"
          % (r["iterations"], len(log), dt, dr))
    assert r["converged"] and 2 <= r["iterations"] < 35
    assert dt < 0.05 and dr < 0.005                                           # a twentieth of a leaf, 0.3 degrees


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, dp, fp, i64p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    want = {
        "ndt_set_source_distributions": [vp, vp, vp, C.c_size_t],
        "ndt_set_source_distributions_device": [vp, vp, vp, C.c_size_t],
        "ndt_source_distributions_info": [vp, i64p, i64p],
        "ndt_export_source_distributions": [vp, dp, dp, vp, vp, C.c_size_t],
        "ndt_eval_derivatives_d2d": [vp, dp, C.c_int, C.c_int, dp],
        "ndt_align_d2d": [vp, fp, C.POINTER(pkg.Result)],
    }
    for name in NEW:
        assert re.search(r"\bint(?:64_t)? %s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    assert L.ndt_export_source_distributions.restype is C.c_int64
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for decl in ("int ndt_set_source_distributions(ndt_handle* h, const int32_t* count, const double* moments9, size_t n);",
                 "int ndt_set_source_distributions_device(ndt_handle* h, const int32_t* count, const double* moments9, size_t n);",
                 "int ndt_source_distributions_info(ndt_handle* h, int64_t* n_records, int64_t* n_accepted);",
                 "int64_t ndt_export_source_distributions(ndt_handle* h, double* mean3, double* cov6, int32_t* count, "
                 "int32_t* record_index, size_t cap);",
                 "int ndt_eval_derivatives_d2d(ndt_handle* h, const double* poses6, int K, int compute_hessian, double* out);",
                 "int ndt_align_d2d(ndt_handle* h, const float guess_colmajor[16], ndt_result* out);"):
        assert decl in flat, decl
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    hpp = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    for m in ("setInputSourceDistributions", "computeDerivativesD2D", "alignDistributions", "getSourceDistributions"):
        assert re.search(r"\b%s\s*\(" % m, hpp), m
    for m in ("setSourceDistributions", "setSourceDistributionsDevice", "sourceDistributionsInfo", "getSourceDistributions",
              "computeDerivativesD2D", "evalDerivativesD2D", "alignDistributions"):
        assert callable(getattr(pkg, m)), m
    mk = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "Makefile")).read()
    assert "$(B)/ndt_d2d.o" in mk and "ndt_leaf_device.h" in mk


def test_argument_errors_come_before_the_handle(pkg):
    L = pkg.lib()
    cnt = (C.c_int32 * 2)(7, 9)
    mom = (C.c_double * 18)(*([1.0] * 18))
    poses = (C.c_double * 6)()
    words = (C.c_double * 32)()
    guess = (C.c_float * 16)()
    res = pkg.Result()
    a, b = C.c_int64(5), C.c_int64(6)
    # NULL handle
    assert L.ndt_set_source_distributions(None, cnt, mom, 2) == -1
    assert L.ndt_set_source_distributions_device(None, cnt, mom, 2) == -1
    assert L.ndt_source_distributions_info(None, C.byref(a), C.byref(b)) == -1 and (a.value, b.value) == (5, 6)
    assert L.ndt_export_source_distributions(None, None, None, None, None, 0) == -1
    assert L.ndt_eval_derivatives_d2d(None, poses, 1, 1, words) == -1
    assert L.ndt_align_d2d(None, guess, C.byref(res)) == -1
    # the argument checks come before the handle is looked at: a stand-in block of zero bytes is never read
    h = C.create_string_buffer(1 << 16)
    for fn in (L.ndt_set_source_distributions, L.ndt_set_source_distributions_device):
        assert fn(h, None, mom, 2) == -1
        assert fn(h, cnt, None, 2) == -1
    zero = (C.c_int32 * 2)(7, 0)
    assert L.ndt_set_source_distributions(h, zero, mom, 2) == -1                     # count < 1
    for bad in (np.nan, np.inf, -np.inf):
        m2 = (C.c_double * 18)(*([1.0] * 18))
        m2[13] = bad
        assert L.ndt_set_source_distributions(h, cnt, m2, 2) == -1                  # a non-finite moment
    assert L.ndt_eval_derivatives_d2d(h, None, 1, 1, words) == -1
    assert L.ndt_eval_derivatives_d2d(h, poses, 1, 1, None) == -1
    assert L.ndt_eval_derivatives_d2d(h, poses, 0, 1, words) == -1
    nan_pose = (C.c_double * 6)(0, 0, 0, 0, np.nan, 0)
    assert L.ndt_eval_derivatives_d2d(h, nan_pose, 1, 1, words) == -1
    assert L.ndt_align_d2d(h, None, C.byref(res)) == -1
    assert L.ndt_align_d2d(h, guess, None) == -1
    assert bytes(h.raw) == bytes(1 << 16) and not any(words)                        # nothing was written


def test_python_mirror_validates_before_the_library(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)   # no handle: nothing may reach the library
    ndt._h = None
    bad = [
        lambda: pkg.setSourceDistributions(ndt),
        lambda: pkg.setSourceDistributions(ndt, dict(count=np.ones(2), moments=None)),
        lambda: pkg.setSourceDistributions(ndt, count=np.ones(3), moments=np.zeros((2, 9))),
        lambda: pkg.setSourceDistributions(ndt, count=np.ones(2), moments=np.zeros((2, 6))),
        lambda: pkg.setSourceDistributions(ndt, count=np.ones((2, 1)), moments=np.zeros((2, 9))),
        lambda: pkg.setSourceDistributionsDevice(ndt, 0, 16, 4),
        lambda: pkg.setSourceDistributionsDevice(ndt, 16, None, 4),
        lambda: pkg.evalDerivativesD2D(ndt, np.zeros(5)),
        lambda: pkg.evalDerivativesD2D(ndt, np.full((2, 6), np.nan)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d reached the library" % k)


# ---- the kernels --------------------------------------------------------------------------------------------------------
def test_d2d_kernels_do_not_spill(tmp_path):
    """The figures tools/kernel_resources.py prints for `ndt_d2d.hip k_d2d_` and for the fixed-order sum it shares with the
    continuous-time evaluation (`ndt_eval_rows.hip k_eval_rows_`): every kernel without scratch, the Hessian
    instantiations of k_d2d_eval within the 256 architectural VGPRs."""
    def resources(file_name):
        path = os.path.join(ROOT, "slam-sam_amd", "csrc", file_name)
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
        return path, usage

    _, rows_usage = resources("ndt_eval_rows.hip")
    assert len(rows_usage) == 1 and "k_eval_rows_sum" in next(iter(rows_usage)), sorted(rows_usage)
    path, usage = resources("ndt_d2d.hip")
    assert usage and all("k_d2d_" in k for k in usage), sorted(usage)                 # the new kernels carry the prefix
    assert not any("k_derivatives" in k for k in usage)
    kernels = {re.search(r"k_d2d_[a-z_]+?(?=I|E)", k).group(0) for k in usage}
    assert kernels == {"k_d2d_check", "k_d2d_finalize", "k_d2d_emit", "k_d2d_gather_target", "k_d2d_eval"}, kernels
    assert len(usage) == 8                                                            # k_d2d_eval: <HESSIAN, D7> four times
    usage.update(rows_usage)
    for k, u in usage.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 256, (k, u)
    src = open(path).read()
    assert len(re.findall(r"__global__", src)) == len(kernels)
    # no float atomics (one integer atomicOr: the device setter's argument check), no inline assembly; the leaf rule and
    # the compaction are called, not copied
    assert re.findall(r"atomic\w*\(", src) == ["atomicOr("] and not re.search(r"\basm\b", src)
    assert "finalize_leaf(" in src and "jacobi" not in src and '#include "ndt_leaf_device.h"' in src
    assert "compact_ballot(" in src and "compact_position(" in src and "launch_filter_scan(" in src and "compact_total(" in src
    # the neighbour rule, the block row and the host driver are called, not copied
    assert "neighbor_cells7<" in src and "floorf(" not in src and "eval_block_row<" in src and "__shfl_xor" not in src
    assert "lane_eval_rows(" in src and "lane_align(" in src and "finish_words(" in src
    target = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_target.hip")).read()
    assert '#include "ndt_leaf_device.h"' in target and "bool finalize_leaf(" not in target
