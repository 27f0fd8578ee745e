"""CPU checks of GICP (ndt_gicp_default_params / _set_params / _get_params, ndt_gicp_export_neighbours / _covariances,
ndt_gicp_pair, ndt_gicp_export_pairs, ndt_eval_derivatives_gicp, ndt_align_gicp; no GPU): the nine symbols are declared,
exported, listed and bound with ABI version 3 unchanged; arguments are refused before the handle is looked at, and the
Python functions refuse misshapen input before the library is called; the kernels of ndt_gicp.hip compile for gfx950
without scratch, and so do those of ndt_fitness.hip after its device side moved into ndt_fit_device.h.
The NumPy yardstick the GPU tests compare with lives here, the rule of include/ndt_hip.h operation by operation:
`knn_brute` (neighbours by (d2, index) over ALL points, no index structure), `cov_numpy` (the two in-order passes, a loop
over the k columns), `reg_cov_numpy` (the normal by numpy.linalg.eigh), `pairs_brute`, `gicp_numpy` (the D2D rule's q_a and
q_ab as test_d2d_cpu.d2d_numpy writes them, weight -1/2, no q_a q_b term) and `gicp_align_numpy` (the two-level loop over
ndt_newton_align).  Its own checks: gradient and Hessian against central differences, and that the test clouds produce
every case the GPU tests are meant to meet."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from test_ct_cpu import scene
from test_d2d_cpu import FD_STEP, FD_TOL, KW, moved_means, rot_derivs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_gicp_default_params", "ndt_gicp_set_params", "ndt_gicp_get_params", "ndt_gicp_export_neighbours",
       "ndt_gicp_export_covariances", "ndt_gicp_pair", "ndt_gicp_export_pairs", "ndt_eval_derivatives_gicp", "ndt_align_gicp")
SIZES = (3, 19, 20, 63, 64, 257, 1000, 4099)       # fewer points than k, a partial wave, a full wave, one past a block, many blocks
KS = (4, 20, 32)
MIN_NEIGHBOURS = 4
GAP_MIN, GAP_SHARE = 1e-3, 0.05                    # the regularised covariance is compared where (l1 - l0) / l2 >= GAP_MIN
DEFAULTS = dict(k_neighbours=20, max_neighbour_distance=np.inf, covariance_epsilon=1e-3, max_correspondence_distance=5.0,
                transformation_epsilon=1e-4, max_iterations=64, max_inner_iterations=20)


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def knn_brute(cloud, k, cap=np.inf, chunk=512):
    """(idx [n, k] int32 in (d2, index) order, -1 padded; n_found [n] int32): d2 = (dx*dx + dy*dy) + dz*dz in f32 between
    every pair of finite points of the cloud, the point itself included; with a finite cap only d2 <= (float)(cap * cap)"""
    p = np.ascontiguousarray(cloud, np.float32)
    n = len(p)
    finite = np.isfinite(p).all(axis=1)
    cap2 = np.float32(np.float64(cap) * np.float64(cap))
    idx, found = np.full((n, k), -1, np.int32), np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for a in range(0, n, chunk):
            q = p[a:a + chunk]
            dx, dy, dz = (p[None, :, c] - q[:, None, c] for c in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz                                # float32 throughout
            out = ~finite[None, :] | ~finite[a:a + chunk, None] | (d2 > cap2)
            key = np.where(out, np.float32(np.nan), d2)                       # NaN sorts last; stable: ties by index
            order = np.argsort(key, axis=1, kind="stable")[:, :k]
            m = np.minimum((~out).sum(axis=1), k)
            take = np.arange(order.shape[1])[None, :] < m[:, None]
            idx[a:a + chunk, :order.shape[1]] = np.where(take, order, -1)
            found[a:a + chunk] = m
    return idx, found


def cov_numpy(cloud, idx, found):
    """(mean [n, 3], raw6 [n, 6]) in f64: sums taken sequentially over the list, column by column; NaN rows for m < 4"""
    x = np.ascontiguousarray(cloud, np.float32).astype(np.float64)
    n, k = idx.shape
    safe = np.where(idx >= 0, idx, 0)
    s = np.zeros((n, 3))
    for j in range(k):
        live = (j < found)[:, None]
        s = np.where(live, s + x[safe[:, j]], s)
    m = found.astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        mean = s / m
        c = np.zeros((n, 6))
        for j in range(k):
            live = (j < found)[:, None]
            d = x[safe[:, j]] - mean
            prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                             d[:, 2] * d[:, 2]], axis=1)
            c = np.where(live, c + prod, c)
        raw = c / m
    none = found < MIN_NEIGHBOURS
    mean[none] = np.nan
    raw[none] = np.nan
    return mean, raw


def sym3(c6):
    return np.asarray(c6)[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def reg_cov_numpy(raw6, eps):
    """(C [n, 3, 3] = I - (1 - eps) n n^T with n from numpy.linalg.eigh, relative gap (l1 - l0) / l2 [n]); NaN rows stay NaN"""
    A = sym3(raw6)
    ok = np.isfinite(A).all(axis=(1, 2))
    w, V = np.linalg.eigh(np.where(ok[:, None, None], A, np.eye(3)))
    nrm = V[:, :, 0]
    Cm = np.eye(3)[None] - (1.0 - eps) * nrm[:, :, None] * nrm[:, None, :]
    with np.errstate(all="ignore"):
        gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    Cm[~ok] = np.nan
    gap[~ok] = np.nan
    return Cm, gap


def moved_points(pose6, src):
    """x' of the rule in f64 (the D2D rule's moved mean) for the f32 points src"""
    return moved_means(np.asarray(pose6, np.float64), np.ascontiguousarray(src, np.float32).astype(np.float64))


def pairs_brute(pose6, src, src_found, tgt, tgt_found, D, chunk=512):
    """(target_index [n] int32, d2 [n] float32): the finite target point with the smallest (d2, index) from the f32 rounding
    of the moved point; kept when d2 <= (float)(D * D) and both points have a covariance, else -1 / +inf"""
    with np.errstate(all="ignore"):
        q = moved_points(pose6, src).astype(np.float32)
    t = np.ascontiguousarray(tgt, np.float32)
    tfin = np.isfinite(t).all(axis=1)
    cap2 = np.float32(np.float64(D) * np.float64(D))
    n = len(q)
    out_i, out_d = np.full(n, -1, np.int32), np.full(n, np.inf, np.float32)
    with np.errstate(all="ignore"):
        for a in range(0, n, chunk):
            qq = q[a:a + chunk]
            dx, dy, dz = (t[None, :, c] - qq[:, None, c] for c in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            key = np.where(tfin[None, :], d2, np.float32(np.inf))
            best = np.argmin(key, axis=1)                                     # the first of equal minima: the lowest index
            bd = key[np.arange(len(qq)), best]
            live = (src_found[a:a + chunk] >= MIN_NEIGHBOURS) & np.isfinite(qq).all(axis=1) & tfin[best]
            keep = live & (bd <= cap2) & (tgt_found[best] >= MIN_NEIGHBOURS)
            out_i[a:a + chunk] = np.where(keep, best, -1)
            out_d[a:a + chunk] = np.where(keep, bd, np.float32(np.inf))
    return out_i, out_d


def gicp_numpy(pose6, src_pts, src_cov, tgt_pts, tgt_cov, pair, hessian=True):
    """The evaluation rule over frozen pairs: dict(score, gradient [6], hessian [6, 6], nvtl_sum, n_with_neighbors,
    n_pairs).  src_pts / tgt_pts: f32 points; src_cov / tgt_cov: [n, 3, 3] regularised covariances; pair [n]: target index
    or -1.  q_a and q_ab are the D2D rule's (test_d2d_cpu.d2d_numpy), the weight is -1/2 and there is no q_a q_b term."""
    pose6 = np.asarray(pose6, np.float64)
    R, dR, d2R = rot_derivs(pose6)
    x = np.ascontiguousarray(src_pts, np.float32).astype(np.float64)
    b = np.ascontiguousarray(tgt_pts, np.float32).astype(np.float64)
    pi = np.nonzero(np.asarray(pair) >= 0)[0]
    ps = np.asarray(pair)[pi]
    out = dict(score=0.0, gradient=np.zeros(6), hessian=np.zeros((6, 6)), nvtl_sum=0.0, n_with_neighbors=0, n_pairs=0)
    if len(pi) == 0:
        return out
    S = np.asarray(src_cov, np.float64)[pi]
    xi = x[pi]
    m = moved_means(pose6, xi)
    mu = m - b[ps]
    A = np.einsum("ab,nbc,dc->nad", R, S, R)
    with np.errstate(all="ignore"):
        B = np.linalg.inv(A + np.asarray(tgt_cov, np.float64)[ps])
        v = np.einsum("pab,pb->pa", B, mu)
        q = np.einsum("pa,pa->p", mu, v)
    ok = np.isfinite(q)
    pi, ps, S, xi, B, v, q = pi[ok], ps[ok], S[ok], xi[ok], B[ok], v[ok], q[ok]
    P = len(pi)
    score = float((-0.5 * q).sum())
    out.update(score=score, nvtl_sum=score, n_with_neighbors=P, n_pairs=P)
    j = np.zeros((P, 6, 3))
    Z = np.zeros((P, 6, 3, 3))
    j[:, :3] = np.eye(3)
    for c in range(3):
        j[:, 3 + c] = xi @ dR[c].T
        M = np.einsum("ab,nbc,dc->nad", dR[c], S, R)
        Z[:, 3 + c] = M + M.transpose(0, 2, 1)
    Bj = np.einsum("pab,pkb->pka", B, j)
    Zv = np.einsum("pkab,pb->pka", Z, v)
    qa = 2.0 * np.einsum("pa,pka->pk", v, j) - np.einsum("pa,pka->pk", v, Zv)
    out["gradient"] = (-0.5 * qa).sum(axis=0)
    if not hessian:
        return out
    BZv = np.einsum("pab,pkb->pka", B, Zv)
    qab = (2.0 * np.einsum("pbx,pax->pab", j, Bj) - 2.0 * np.einsum("pbx,pax->pab", Zv, Bj)
           - 2.0 * np.einsum("pbx,pax->pab", j, BZv) + 2.0 * np.einsum("pbx,pax->pab", Zv, BZv))
    for c in range(3):
        for d in range(3):
            Hcd = xi @ d2R[c][d].T
            N = np.einsum("ab,nbc,dc->nad", d2R[c][d], S, R) + np.einsum("ab,nbc,dc->nad", dR[c], S, dR[d])
            Zcd = N + N.transpose(0, 2, 1)
            qab[:, 3 + c, 3 + d] += 2.0 * np.einsum("pa,pa->p", v, Hcd) - np.einsum("pa,pab,pb->p", v, Zcd, v)
    out["hessian"] = (-0.5 * qab).sum(axis=0)
    return out


def gicp_align_numpy(pkg, src, src_cov, src_found, tgt, tgt_cov, tgt_found, guess, prm=None, **ndt_kw):
    """ndt_align_gicp's two-level loop on the CPU: pairs_brute at the current pose, ndt_newton_align over gicp_numpy with the
    frozen pairs.  Returns dict(T, pose, converged, outer, inner [per outer iteration], n_pairs)."""
    g = dict(DEFAULTS, **(prm or {}))
    params = pkg.default_params(resolution=1.0, **dict(dict(KW, **ndt_kw), trans_epsilon=g["transformation_epsilon"],
                                                       max_iterations=g["max_inner_iterations"]))
    T = np.asarray(guess, np.float64).astype(np.float32).astype(np.float64)
    # p_0: the pose ndt_newton_align derives from the guess matrix -- a loop whose first evaluation has no gradient stops there
    p = np.asarray(pkg.newton_align(params, len(src), T, lambda pose6, Tm, need_h: pkg.pack_eval(0.0, np.zeros(6), -np.eye(6)))["pose"])
    inner, converged, n_pairs = [], False, 0
    while len(inner) < g["max_iterations"] and not converged:
        pair, _ = pairs_brute(p, src, src_found, tgt, tgt_found, g["max_correspondence_distance"])
        n_pairs = int((pair >= 0).sum())
        assert n_pairs > 0

        def ev(pose6, Tm, need_h, pair=pair):
            r = gicp_numpy(pose6, src, src_cov, tgt, tgt_cov, pair, hessian=bool(need_h))
            return pkg.pack_eval(r["score"], r["gradient"], r["hessian"], r["nvtl_sum"], r["n_with_neighbors"], r["n_pairs"])

        r = pkg.newton_align(params, len(src), T, ev)
        inner.append(r["iterations"])
        q = np.asarray(r["pose"], np.float64)
        converged = float(np.sqrt(((q - p) ** 2).sum())) < g["transformation_epsilon"]
        p, T = q, np.asarray(r["T"], np.float64)
    return dict(T=T, pose=p, converged=converged, outer=len(inner), inner=inner, n_pairs=n_pairs)


# ---- the test clouds ----------------------------------------------------------------------------------------------------
FAR = np.array([500.0, 1.0, 1.0], np.float32)


def knn_cloud(n):
    """n points (float32) that carry the hard cases: an integer lattice of spacing 1 (many equal d2: the tie rule decides;
    with the index's cell edge of 1 m every point lies on a cell face), duplicates of lattice points, one point with a NaN
    coordinate (n >= 3) and one point 500 m away (n >= 19)."""
    side = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)
    p = np.random.default_rng(n).permutation(g)[:n].astype(np.float32)
    if n >= 3:
        p[1, 1] = np.nan
    if n >= 19:
        p[n // 2] = p[0]                                                     # duplicates: equal d2 to everything
        p[n // 3] = p[n - 2]
        p[n - 1] = FAR
    return p


@functools.lru_cache(maxsize=None)
def scene_neighbours(which, k=20):
    """brute-force neighbours and covariances of the scene's target / rigid scan, computed once"""
    s = scene()
    cloud = s["target"] if which == "target" else s["ideal"]
    idx, found = knn_brute(cloud, k)
    mean, raw = cov_numpy(cloud, idx, found)
    Cm, gap = reg_cov_numpy(raw, DEFAULTS["covariance_epsilon"])
    return dict(cloud=cloud, idx=idx, found=found, mean=mean, raw=raw, cov=Cm, gap=gap)


# ---- the yardstick's own checks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_the_clouds_produce_every_case(n):
    """brute force alone: equal d2 decided by the index, duplicates, a NaN point, the far point, and under a finite cap of
    1 m points with fewer than 4 neighbours beside points with more"""
    p = knn_cloud(n)
    for k in KS:
        idx, found = knn_brute(p, k)
        fin = np.isfinite(p).all(axis=1)
        assert found[~fin].sum() == 0 and (idx[~fin] == -1).all()
        assert (found[fin] == min(k, int(fin.sum()))).all()
        assert (idx[fin, 0] <= np.nonzero(fin)[0]).all()                     # d2 = 0: the point itself or an earlier duplicate
        if n < k:
            assert (idx[:, -1] == -1).all()                                   # fewer points than k: padded
    if n >= 3:
        assert not np.isfinite(p[1]).all()
    if n >= 19:
        idx, found = knn_brute(p, 20)
        x = p.astype(np.float64)
        safe = np.where(idx >= 0, idx, 0)
        d2 = ((x[safe] - x[:, None, :]) ** 2).sum(axis=2)
        ties = (np.diff(d2, axis=1) == 0) & (idx[:, 1:] >= 0)
        assert ties.sum() > n // 2                                            # many equal d2 ...
        assert (np.diff(idx, axis=1)[ties] > 0).all()                         # ... in index order
        assert idx[n // 2, 0] == 0 and idx[0, 1] == n // 2                    # the duplicate pair: lowest index first
        assert (p[n - 1] == FAR).all() and d2[n - 1, 1] > 400.0 ** 2          # the far point's neighbours are all far
        _, f1 = knn_brute(p, 20, cap=1.0)
        assert (f1[fin] < MIN_NEIGHBOURS).any() and (f1 >= MIN_NEIGHBOURS).any() and f1[n - 1] == 1
    else:
        _, f1 = knn_brute(p, 20, cap=1.0)
        assert (f1 < MIN_NEIGHBOURS).all()


def test_the_scene_stays_within_the_gap_share(pkg):
    """at most 5 % of the scene's points have their two smallest eigenvalues closer than 1e-3 of the largest"""
    for which in ("target", "source"):
        s = scene_neighbours(which)
        assert (s["found"] == 20).all()
        share = float((s["gap"] < GAP_MIN).mean())
        print("%s: %.4f of the points below the gap" % (which, share))
        assert share <= GAP_SHARE
        C3 = s["cov"]
        assert np.abs(np.trace(C3, axis1=1, axis2=2) - (2.0 + 1e-3)).max() < 1e-12


def test_gradient_and_hessian_are_the_central_differences(pkg):
    """step and bound as tests/test_d2d_cpu.py derives them for the same check: the terms are the same q, here without the
    exponential, so third derivatives come from the rotation alone and rounding of the sums is far below the bound"""
    from slam_sam_amd import synth
    S, Tg = scene_neighbours("source"), scene_neighbours("target")
    for attitude in ((0.0, 0.0, 0.0), (0.02, -0.03, 0.6)):
        pose = np.array([0.07, -0.05, 0.03, *attitude])
        back = np.linalg.inv(synth.pose_matrix(0, 0, 0, *attitude))
        src = synth.transform(back, S["cloud"]).astype(np.float32)
        Rb = back[:3, :3]
        cov = np.einsum("ab,nbc,dc->nad", Rb, S["cov"], Rb)
        pair, _ = pairs_brute(pose, src, S["found"], Tg["cloud"], Tg["found"], 5.0)
        assert (pair >= 0).sum() > 4000
        at = gicp_numpy(pose, src, cov, Tg["cloud"], Tg["cov"], pair)
        assert at["score"] < 0 and at["n_pairs"] == (pair >= 0).sum()
        assert np.abs(at["hessian"] - at["hessian"].T).max() <= 1e-12 * np.abs(at["hessian"]).max()
        g_fd, H_fd = np.zeros(6), np.zeros((6, 6))
        for a in range(6):
            hi, lo = pose.copy(), pose.copy()
            hi[a] += FD_STEP
            lo[a] -= FD_STEP
            rh = gicp_numpy(hi, src, cov, Tg["cloud"], Tg["cov"], pair, hessian=False)
            rl = gicp_numpy(lo, src, cov, Tg["cloud"], Tg["cov"], pair, hessian=False)
            g_fd[a] = (rh["score"] - rl["score"]) / (2 * FD_STEP)
            H_fd[a] = (rh["gradient"] - rl["gradient"]) / (2 * FD_STEP)
        eg = np.linalg.norm(at["gradient"] - g_fd) / np.linalg.norm(at["gradient"])
        eh = np.linalg.norm(at["hessian"] - H_fd) / np.linalg.norm(at["hessian"])
        print("central differences %s: gradient %.2e, Hessian %.2e of their norms" % (attitude, eg, eh))
        assert eg < FD_TOL and eh < FD_TOL, (eg, eh)
        no_h = gicp_numpy(pose, src, cov, Tg["cloud"], Tg["cov"], pair, hessian=False)
        assert no_h["score"] == at["score"] and np.array_equal(no_h["gradient"], at["gradient"]) and not no_h["hessian"].any()


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, dp, fp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float)
    gpp = C.POINTER(pkg.GicpParams)
    want = {
        "ndt_gicp_default_params": [gpp],
        "ndt_gicp_set_params": [vp, gpp],
        "ndt_gicp_get_params": [vp, gpp],
        "ndt_gicp_export_neighbours": [vp, C.c_int, vp, vp, C.c_size_t],
        "ndt_gicp_export_covariances": [vp, C.c_int, dp, dp, dp, C.c_size_t],
        "ndt_gicp_pair": [vp, dp, C.POINTER(C.c_int64)],
        "ndt_gicp_export_pairs": [vp, vp, vp, C.c_size_t],
        "ndt_eval_derivatives_gicp": [vp, dp, C.c_int, C.c_int, dp],
        "ndt_align_gicp": [vp, fp, C.POINTER(pkg.Result), C.POINTER(pkg.GicpInfo)],
    }
    for name in NEW:
        assert re.search(r"\b(?:int|int64_t|void)\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    for name in ("ndt_gicp_export_neighbours", "ndt_gicp_export_covariances", "ndt_gicp_export_pairs"):
        assert getattr(L, name).restype is C.c_int64
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for decl in ("void ndt_gicp_default_params(ndt_gicp_params* p);",
                 "int ndt_gicp_set_params(ndt_handle* h, const ndt_gicp_params* p);",
                 "int ndt_gicp_get_params(const ndt_handle* h, ndt_gicp_params* p);",
                 "int64_t ndt_gicp_export_neighbours(ndt_handle* h, int which, int32_t* idx, int32_t* n_found, size_t cap);",
                 "int64_t ndt_gicp_export_covariances(ndt_handle* h, int which, double* mean3, double* raw_cov6, double* cov6, "
                 "size_t cap);",
                 "int ndt_gicp_pair(ndt_handle* h, const double pose6[6], int64_t* n_pairs);",
                 "int64_t ndt_gicp_export_pairs(ndt_handle* h, int32_t* target_index, float* d2, size_t cap);",
                 "int ndt_eval_derivatives_gicp(ndt_handle* h, const double* poses6, int K, int compute_hessian, double* out);",
                 "int ndt_align_gicp(ndt_handle* h, const float guess_colmajor[16], ndt_result* out, ndt_gicp_info* info);"):
        assert decl in flat, decl
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    p = pkg.gicpDefaultParams()
    assert {k: getattr(p, k) for k, _ in pkg.GicpParams._fields_} == DEFAULTS
    hpp = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    assert re.search(r"class GeneralizedIterativeClosestPoint\b", hpp)
    for m in ("setMaxCorrespondenceDistance", "setTransformationEpsilon", "setCorrespondenceRandomness", "setMaximumIterations",
              "setMaximumOptimizerIterations", "setInputSource", "setInputTarget", "align", "getFinalTransformation",
              "hasConverged", "getFitnessScore"):
        assert re.search(r"\b%s\s*\(" % m, hpp), m
    for name in ("gicp_omp.h", "gicp_omp_impl.hpp"):
        txt = open(os.path.join(ROOT, "include", "compat", "pclomp", name)).read()
        assert "gicp_omp.h" in txt
    assert "GeneralizedIterativeClosestPoint" in open(os.path.join(ROOT, "include", "compat", "pclomp", "gicp_omp.h")).read()
    for m in ("gicpSetParams", "gicpGetParams", "gicpNeighbours", "gicpCovariances", "gicpPair", "gicpPairs", "evalDerivativesGICP",
              "alignGICP"):
        assert callable(getattr(pkg, m)), m
    mk = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "Makefile")).read()
    assert "$(B)/ndt_gicp.o" in mk and "ndt_fit_device.h" in mk and "ndt_d2d_device.h" in mk


def test_argument_errors_come_before_the_handle(pkg):
    L = pkg.lib()
    good = pkg.gicpDefaultParams()
    pose = (C.c_double * 6)()
    words = (C.c_double * 32)()
    guess = (C.c_float * 16)()
    idx = (C.c_int32 * 64)()
    d2 = (C.c_float * 4)()
    mean = (C.c_double * 24)()
    res, info, n = pkg.Result(), pkg.GicpInfo(), C.c_int64(7)
    # NULL handle
    assert L.ndt_gicp_set_params(None, C.byref(good)) == -1
    assert L.ndt_gicp_get_params(None, C.byref(good)) == -1
    assert L.ndt_gicp_export_neighbours(None, 0, idx, idx, 2) == -1
    assert L.ndt_gicp_export_covariances(None, 0, mean, mean, mean, 2) == -1
    assert L.ndt_gicp_pair(None, pose, C.byref(n)) == -1 and n.value == 7
    assert L.ndt_gicp_export_pairs(None, idx, d2, 2) == -1
    assert L.ndt_eval_derivatives_gicp(None, pose, 1, 1, words) == -1
    assert L.ndt_align_gicp(None, guess, C.byref(res), C.byref(info)) == -1
    L.ndt_gicp_default_params(None)                                                   # (nothing to fill: no effect)
    # the argument checks come before the handle is looked at: a stand-in block of zero bytes is never read
    h = C.create_string_buffer(1 << 16)
    assert L.ndt_gicp_set_params(h, None) == -1
    assert L.ndt_gicp_get_params(h, None) == -1
    bad_values = dict(k_neighbours=(3, 33, 0, -1), max_neighbour_distance=(0.0, -1.0, np.nan),
                      covariance_epsilon=(0.0, -1e-3, 1.5, np.nan, np.inf), max_correspondence_distance=(0.0, -5.0, np.nan),
                      transformation_epsilon=(-1e-4, np.nan, np.inf), max_iterations=(0, -1), max_inner_iterations=(0, -2))
    for field, values in bad_values.items():
        for v in values:
            p = pkg.gicpDefaultParams()
            setattr(p, field, v)
            assert L.ndt_gicp_set_params(h, C.byref(p)) == -1, (field, v)
    for which in (-1, 2):
        assert L.ndt_gicp_export_neighbours(h, which, idx, idx, 2) == -1
        assert L.ndt_gicp_export_covariances(h, which, mean, mean, mean, 2) == -1
    nan_pose = (C.c_double * 6)(0, 0, 0, 0, np.nan, 0)
    inf_pose = (C.c_double * 6)(np.inf, 0, 0, 0, 0, 0)
    assert L.ndt_gicp_pair(h, None, C.byref(n)) == -1
    assert L.ndt_eval_derivatives_gicp(h, None, 1, 1, words) == -1
    assert L.ndt_eval_derivatives_gicp(h, pose, 1, 1, None) == -1
    assert L.ndt_eval_derivatives_gicp(h, pose, 0, 1, words) == -1
    assert L.ndt_eval_derivatives_gicp(h, pose, -3, 1, words) == -1
    for bad in (nan_pose, inf_pose):
        assert L.ndt_gicp_pair(h, bad, C.byref(n)) == -1
        assert L.ndt_eval_derivatives_gicp(h, bad, 1, 1, words) == -1
    assert L.ndt_align_gicp(h, None, C.byref(res), C.byref(info)) == -1
    assert L.ndt_align_gicp(h, guess, None, C.byref(info)) == -1
    assert bytes(h.raw) == bytes(1 << 16) and not any(words) and n.value == 7         # nothing was written


def test_python_functions_validate_before_the_library(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)   # no handle: nothing may reach the library
    ndt._h = None
    bad = [
        lambda: pkg.gicpSetParams(ndt, k=20),
        lambda: pkg.gicpSetParams(ndt, k_neighbours=20.5),
        lambda: pkg.gicpSetParams(ndt, k_neighbours=True),
        lambda: pkg.gicpSetParams(ndt, covariance_epsilon=np.nan),
        lambda: pkg.gicpSetParams(ndt, max_correspondence_distance=[5.0, 5.0]),
        lambda: pkg.gicpNeighbours(ndt, "both"),
        lambda: pkg.gicpCovariances(ndt, 2),
        lambda: pkg.gicpPair(ndt, np.zeros(5)),
        lambda: pkg.gicpPair(ndt, np.full(6, np.inf)),
        lambda: pkg.evalDerivativesGICP(ndt, np.zeros(5)),
        lambda: pkg.evalDerivativesGICP(ndt, np.full((2, 6), np.nan)),
        lambda: pkg.alignGICP(ndt, np.zeros((3, 3))),
        lambda: pkg.alignGICP(ndt, np.full((4, 4), np.nan)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d reached the library" % k)


# ---- the kernels --------------------------------------------------------------------------------------------------------
def kernel_resources(file_name, tmp_path):
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
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    return path, usage


def test_gicp_kernels_do_not_spill(tmp_path):
    """ndt_gicp.hip for gfx950: every kernel carries k_gicp_, none uses scratch, all stay within the 256 architectural
    VGPRs (the per-lane top-k list is indexed by compile-time indices only); the figures go to profiles/gicp_resources.txt.
    Shared code is called, not copied."""
    path, usage = kernel_resources("ndt_gicp.hip", tmp_path)
    assert usage and all("k_gicp_" in k for k in usage), sorted(usage)
    kernels = {re.search(r"k_gicp_[a-z_]+?(?=I|E)", k).group(0) for k in usage}
    assert kernels == {"k_gicp_knn", "k_gicp_knn_tail", "k_gicp_cov", "k_gicp_pair", "k_gicp_pair_tail", "k_gicp_eval"}, kernels
    assert len(usage) == 13                                          # knn / knn_tail: KMAX 8, 16, 24, 32; eval: with and without Hessian
    lines = ["kernel resources of slam-sam_amd/csrc/ndt_gicp.hip for gfx950 (-O3 -ffp-contract=off; tests/test_gicp_cpu.py writes this file)",
             "%-28s %6s %6s %8s %10s %6s" % ("kernel", "VGPRs", "AGPRs", "scratch", "occupancy", "LDS")]
    for k in sorted(usage):
        u = usage[k]
        short = re.search(r"k_gicp_[a-z_]+?(?=I|E)", k).group(0) + "".join("<%s>" % a for a in re.findall(r"IL[ib](\d+)E", k))
        lines.append("%-28s %6d %6d %8d %10d %6d" % (short, u["VGPRs"], u.get("AGPRs", 0), u["ScratchSize"], u.get("Occupancy", 0),
                                                    u.get("LDS", 0)))
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 256, (k, u)
    print("\n".join(lines))
    with open(os.path.join(ROOT, "profiles", "gicp_resources.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    src = open(path).read()
    assert len(re.findall(r"__global__", src)) == len(kernels)
    # integer atomics only (queue positions and counters), no inline assembly
    assert set(re.findall(r"atomic\w*\(", src)) == {"atomicAdd("} and not re.search(r"\basm\b", src)
    assert "double" not in re.search(r"atomicAdd\([^;]*;", src).group(0)
    # the index's device side, the pair rule, the block row and the host driver are the shared ones
    assert '#include "ndt_fit_device.h"' in src and "fit_lower_bound2(" in src and "fit_walk_shell(" in src and "fit_hash(" not in src
    assert '#include "ndt_d2d_device.h"' in src and "d2d_pair<" in src and "jacobi_rot<" in src
    assert "eval_block_row<" in src and "__shfl_xor" not in src and "lane_eval_rows(" in src and "lane_align(" in src
    d2d = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_d2d.hip")).read()
    assert '#include "ndt_d2d_device.h"' in d2d and "void d2d_pair(" not in d2d


def test_fitness_kernels_still_do_not_spill(tmp_path):
    """ndt_fitness.hip after the header lift: the same seven kernels, none with scratch; the device helpers live in
    ndt_fit_device.h alone"""
    path, usage = kernel_resources("ndt_fitness.hip", tmp_path)
    kernels = {re.search(r"k_fit_[a-z]+", k).group(0) for k in usage}
    assert kernels == {"k_fit_bounds", "k_fit_keys", "k_fit_gather", "k_fit_ends", "k_fit_query", "k_fit_shells", "k_fit_reduce"}
    for k, u in usage.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 256, (k, u)
    src = open(path).read()
    assert '#include "ndt_fit_device.h"' in src and "float fit_lower_bound2(" not in src and "fit_build_cloud(" in src
    hdr = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_fit_device.h")).read()
    assert "float fit_lower_bound2(" in hdr and "fit_walk_shell(" in hdr
