"""CPU checks of voxelised GICP (ndt_vgicp_export_voxels, ndt_vgicp_get_info, ndt_eval_derivatives_vgicp, ndt_align_vgicp;
no GPU): the four symbols are declared, exported, listed and bound with ABI version 3 unchanged; arguments are refused
before the handle is looked at, and the Python functions refuse misshapen input before the library is called; the kernels
of ndt_vgicp.hip compile for gfx950 without scratch.
The NumPy yardstick the GPU tests compare with lives here, the rule of include/ndt_hip.h operation by operation:
`vgicp_voxels_numpy` (the f32 classification of test_d2d_cpu.classify, the sequential f64 sums per leaf in ascending input
index) and `vgicp_numpy` (the neighbour rule of test_d2d_cpu.d2d_pairs, the D2D rule's q_a and q_ab as
test_gicp_cpu.gicp_numpy writes them, the weight -N / 2, no q_a q_b term).  Its own checks: gradient and Hessian against
central differences, the conditions that keep the GPU tests from passing on nothing, and the host Newton loop
(ndt_newton_align) driven by it.
Scene (test_ct_cpu.scene): 9 000 target points, the rigid 4 500-point scan, the CT test's guess (0.1 m / 0.5 degrees off)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_ct_cpu import GUESS_OFF, P_TRUE, oracle_grid, scene
from test_d2d_cpu import ATTITUDE, FD_STEP, FD_TOL, KW, classify, d2d_pairs, moved_means, rot_derivs
from test_gicp_cpu import MIN_NEIGHBOURS, kernel_resources, scene_neighbours, sym3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_vgicp_export_voxels", "ndt_vgicp_get_info", "ndt_eval_derivatives_vgicp", "ndt_align_vgicp")
GUESS_POSE = P_TRUE + GUESS_OFF


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def upper6(cov):
    """xx, xy, xz, yy, yz, zz of [n, 3, 3] covariances"""
    return np.ascontiguousarray(np.asarray(cov, np.float64)[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]])


def vgicp_voxels_numpy(target, cov, found, leaves, grid):
    """The voxel table: dict(count [L] int32, mean [L, 3], cov6 [L, 6], cov [L, 3, 3], n_target_points_in_voxels), one row per
    leaf of `leaves` (dict with `cell` ascending -- getLeaves() or the oracle's export).  target: f32 points; cov [n, 3, 3]:
    their regularised covariances; found [n]: neighbours found (a point with fewer than 4 has no covariance).  A point
    contributes to the leaf whose cell its f32 classification gives; the sums run over a leaf's points in ascending input
    index, in f64, starting from 0; N = 0 gives a NaN row."""
    t = np.ascontiguousarray(target, np.float32)
    cells = np.asarray(leaves["cell"], np.int64)
    L = len(cells)
    cell = classify(t, grid)
    at = np.clip(np.searchsorted(cells, cell), 0, max(L - 1, 0))
    ok = np.isfinite(t).all(axis=1) & (np.asarray(found) >= MIN_NEIGHBOURS) & (cell >= 0) & (L > 0)
    ok &= cells[at] == cell if L else False
    idx = np.nonzero(ok)[0]
    leaf = at[idx]
    order = np.argsort(leaf, kind="stable")                                   # by leaf, ascending input index within one
    idx, leaf = idx[order], leaf[order]
    count = np.bincount(leaf, minlength=L).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    x, c6 = t.astype(np.float64), upper6(cov)
    s, c = np.zeros((L, 3)), np.zeros((L, 6))
    for r in range(int(count.max()) if L else 0):                             # the r-th point of every leaf that has one
        live = count > r
        j = idx[start[live] + r]
        s[live] = s[live] + x[j]
        c[live] = c[live] + c6[j]
    with np.errstate(all="ignore"):
        mean, cov6 = s / count.astype(np.float64)[:, None], c / count.astype(np.float64)[:, None]
    mean[count == 0] = np.nan
    cov6[count == 0] = np.nan
    return dict(count=count, mean=mean, cov6=cov6, cov=sym3(cov6), n_target_points_in_voxels=int(len(idx)))


def vgicp_pairs(pose6, src, src_found, voxels, leaves, grid, method="DIRECT7"):
    """(source index, voxel row) of every pair at pose6, source-major and in probe order: the leaves of the f32-rounded moved
    point (d2d_pairs), for source points with a covariance and voxels with N >= 1"""
    x = np.ascontiguousarray(src, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        m = moved_means(np.asarray(pose6, np.float64), x)
        pi, ps = d2d_pairs(m, leaves, grid, method)
    keep = (np.asarray(src_found)[pi] >= MIN_NEIGHBOURS) & (np.asarray(voxels["count"])[ps] >= 1)
    return pi[keep], ps[keep]


def vgicp_numpy(pose6, src, src_cov, src_found, voxels, leaves, grid, method="DIRECT7", hessian=True, pairs=None):
    """The evaluation rule: dict(score, gradient [6], hessian [6, 6], nvtl_sum, n_with_neighbors, n_pairs).  src: f32 points;
    src_cov [n, 3, 3]; src_found [n]; voxels: the table (vgicp_voxels_numpy or vgicpVoxels()); leaves / grid: getLeaves() /
    getGridInfo() or the oracle's.  pairs: a fixed pair list (central differences).  Per pair f = -N / 2: score += f q,
    gradient += f q_a, Hessian += f q_ab with the D2D rule's q_a and q_ab."""
    pose6 = np.asarray(pose6, np.float64)
    R, dR, d2R = rot_derivs(pose6)
    x = np.ascontiguousarray(src, np.float32).astype(np.float64)
    pi, ps = vgicp_pairs(pose6, src, src_found, voxels, leaves, grid, method) if pairs is None else pairs
    out = dict(score=0.0, gradient=np.zeros(6), hessian=np.zeros((6, 6)), nvtl_sum=0.0, n_with_neighbors=0, n_pairs=0)
    if len(pi) == 0:
        return out
    S = np.asarray(src_cov, np.float64)[pi]
    xi = x[pi]
    m = moved_means(pose6, xi)
    mu = m - np.asarray(voxels["mean"], np.float64)[ps]
    A = np.einsum("ab,nbc,dc->nad", R, S, R)
    with np.errstate(all="ignore"):
        B = np.linalg.inv(A + np.asarray(voxels["cov"], np.float64)[ps])
        v = np.einsum("pab,pb->pa", B, mu)
        q = np.einsum("pa,pa->p", mu, v)
    ok = np.isfinite(q)
    pi, ps, S, xi, B, v, q = pi[ok], ps[ok], S[ok], xi[ok], B[ok], v[ok], q[ok]
    P = len(pi)
    f = -0.5 * np.asarray(voxels["count"], np.float64)[ps]
    score = float((f * q).sum())
    out.update(score=score, nvtl_sum=score, n_with_neighbors=len(np.unique(pi)), n_pairs=P)
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
    out["gradient"] = (f[:, None] * qa).sum(axis=0)
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
    out["hessian"] = (f[:, None, None] * qab).sum(axis=0)
    return out


def restatement_evaluator(pkg, src, src_cov, src_found, voxels, leaves, grid, method, log=None):
    def ev(pose6, T, need_h):
        r = vgicp_numpy(pose6, src, src_cov, src_found, voxels, leaves, grid, method, hessian=bool(need_h))
        if log is not None:
            log.append(np.array(pose6))
        return pkg.pack_eval(r["score"], r["gradient"], r["hessian"], r["nvtl_sum"], r["n_with_neighbors"], r["n_pairs"])
    return ev


def vgicp_align_numpy(pkg, src, src_cov, src_found, voxels, leaves, grid, method, guess, log=None, **ndt_kw):
    """ndt_align_vgicp on the CPU: one run of ndt_newton_align over vgicp_numpy with the engine's parameters"""
    ev = restatement_evaluator(pkg, src, src_cov, src_found, voxels, leaves, grid, method, log=log)
    return pkg.newton_align(pkg.default_params(resolution=1.0, **dict(KW, **ndt_kw)), len(src), guess, ev)


# ---- the scene ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def side(O, pkg):
    """the scene, the oracle's leaves of its target, brute-force covariances of both clouds and the restatement's table"""
    s = scene()
    _, leaves, grid = oracle_grid(O, s["target"])
    T, S = scene_neighbours("target"), scene_neighbours("source")
    voxels = vgicp_voxels_numpy(s["target"], T["cov"], T["found"], leaves, grid)
    return dict(s, leaves=leaves, grid=grid, T=T, S=S, voxels=voxels)


# ---- the yardstick's own checks -----------------------------------------------------------------------------------------
def test_the_scene_gives_the_gpu_tests_something_to_check(side):
    """Conditions on the restatement alone: at least half of the target's points lie in voxels, at least half of the source
    points have a counted pair at the guess under DIRECT1, and the leaf counts sum to n_target_points_in_voxels."""
    v, S = side["voxels"], side["S"]
    n_t, n_s = len(side["target"]), len(side["ideal"])
    share_t = v["n_target_points_in_voxels"] / n_t
    assert int(v["count"].sum()) == v["n_target_points_in_voxels"]
    assert len(v["count"]) == len(side["leaves"]["cell"]) and (v["count"] >= 1).all()   # every leaf of this scene is a voxel
    assert np.isfinite(v["mean"]).all() and np.isfinite(v["cov6"]).all()
    out = {}
    for method in ("DIRECT1", "DIRECT7"):
        r = vgicp_numpy(GUESS_POSE, side["ideal"], S["cov"], S["found"], v, side["leaves"], side["grid"], method)
        out[method] = (r["n_with_neighbors"] / n_s, r["n_pairs"])
        assert r["score"] < 0 and r["n_pairs"] >= r["n_with_neighbors"]
    print("%d voxels hold %.4f of the target points; source points with a pair at the guess: DIRECT1 %.4f (%d pairs), DIRECT7 %.4f (%d pairs)"
          % (len(v["count"]), share_t, out["DIRECT1"][0], out["DIRECT1"][1], out["DIRECT7"][0], out["DIRECT7"][1]))
    assert share_t >= 0.5
    assert out["DIRECT1"][0] >= 0.5
    assert out["DIRECT7"][0] >= out["DIRECT1"][0] and out["DIRECT7"][1] > out["DIRECT1"][1]
    # a voxel's mean lies in (or on the face of) its own cell, its covariance has trace 2 + eps like every point's
    assert np.abs(np.trace(v["cov"], axis1=1, axis2=2) - (2.0 + 1e-3)).max() < 1e-12
    assert np.array_equal(classify(v["mean"].astype(np.float32), side["grid"]), np.asarray(side["leaves"]["cell"], np.int64)) or \
        (classify(v["mean"].astype(np.float32), side["grid"]) == np.asarray(side["leaves"]["cell"], np.int64)).mean() > 0.99


def test_voxel_table_handles_the_special_points(side):
    """a NaN point, a point without a covariance and a leaf none of whose points has one: counted out, NaN row"""
    s, T = side, side["T"]
    found = T["found"].copy()
    cells = classify(s["target"], s["grid"])
    lone = int(np.asarray(s["leaves"]["cell"])[3])
    found[cells == lone] = 0                                                  # every point of leaf 3 loses its covariance
    tgt = s["target"].copy()
    other = int(np.nonzero(cells == int(np.asarray(s["leaves"]["cell"])[5]))[0][0])
    tgt[other, 1] = np.nan                                                    # a point of leaf 5 is not finite
    v = vgicp_voxels_numpy(tgt, T["cov"], found, s["leaves"], s["grid"])
    base = s["voxels"]
    assert v["count"][3] == 0 and np.isnan(v["mean"][3]).all() and np.isnan(v["cov6"][3]).all()
    assert v["count"][5] == base["count"][5] - 1
    rest = np.ones(len(v["count"]), bool)
    rest[[3, 5]] = False
    assert np.array_equal(v["count"][rest], base["count"][rest]) and np.array_equal(v["mean"][rest], base["mean"][rest])
    assert int(v["count"].sum()) == v["n_target_points_in_voxels"] == base["n_target_points_in_voxels"] - base["count"][3] - 1
    # a voxel with N = 0 never pairs
    S = s["S"]
    pi, ps = vgicp_pairs(GUESS_POSE, s["ideal"], S["found"], v, s["leaves"], s["grid"], "DIRECT7")
    assert len(pi) > 0 and not (ps == 3).any()


# Central differences, step and bound as tests/test_d2d_cpu.py derives them: truncation h^2 / 6 times the third derivative,
# rounding about eps |f| / h.  Here every term is f q with a constant f = -N / 2 and q = mu^T B mu, B depending on the pose
# through R C_i R^T alone: no exponential, so third derivatives come from the rotation and the lever arm (<= 20 m here)
# only, a few hundred times the first -- h^2 / 6 of that is ~1e-8 at h = 1e-5.  |f| sums ~1e4 terms of size N q / 2 <~ 1e2:
# eps |f| / h ~ 1e-5 absolute against gradient components of 1e3 .. 1e5.  The bound is test_d2d_cpu's 1e-5 of the norm.
@pytest.mark.parametrize("attitude", [(0.0, 0.0, 0.0), ATTITUDE], ids=["identity", "attitude"])
@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT1"])
def test_gradient_and_hessian_are_the_central_differences(side, attitude, method):
    from slam_sam_amd import synth
    S, v = side["S"], side["voxels"]
    nominal = np.array([*P_TRUE[:3], *attitude])
    # the scan put where `nominal` moves it onto the target, its covariances turned with it
    back = np.linalg.inv(synth.pose_matrix(*nominal)) @ side["truth"]
    src = synth.transform(back, side["ideal"]).astype(np.float32)
    Rb = back[:3, :3]
    cov = np.einsum("ab,nbc,dc->nad", Rb, S["cov"], Rb)
    pose = nominal + np.array([0.07, -0.05, 0.03, 0.004, -0.003, 0.006])
    pairs = vgicp_pairs(pose, src, S["found"], v, side["leaves"], side["grid"], method)
    assert len(pairs[0]) > (8000 if method == "DIRECT7" else 2000)
    args = (src, cov, S["found"], v, side["leaves"], side["grid"], method)
    at = vgicp_numpy(pose, *args, pairs=pairs)
    assert at["score"] < 0 and at["n_pairs"] == len(pairs[0])
    assert np.abs(at["hessian"] - at["hessian"].T).max() <= 1e-12 * np.abs(at["hessian"]).max()
    g_fd, H_fd = np.zeros(6), np.zeros((6, 6))
    for a in range(6):
        hi, lo = pose.copy(), pose.copy()
        hi[a] += FD_STEP
        lo[a] -= FD_STEP
        rh = vgicp_numpy(hi, *args, hessian=False, pairs=pairs)
        rl = vgicp_numpy(lo, *args, hessian=False, pairs=pairs)
        assert rh["n_pairs"] == rl["n_pairs"] == at["n_pairs"]
        g_fd[a] = (rh["score"] - rl["score"]) / (2 * FD_STEP)
        H_fd[a] = (rh["gradient"] - rl["gradient"]) / (2 * FD_STEP)
    eg = np.linalg.norm(at["gradient"] - g_fd) / np.linalg.norm(at["gradient"])
    eh = np.linalg.norm(at["hessian"] - H_fd) / np.linalg.norm(at["hessian"])
    print("central differences %s %s: gradient %.2e, Hessian %.2e of their norms" % (method, attitude, eg, eh))
    assert eg < FD_TOL and eh < FD_TOL, (eg, eh)
    no_h = vgicp_numpy(pose, *args, hessian=False, pairs=pairs)
    assert no_h["score"] == at["score"] and np.array_equal(no_h["gradient"], at["gradient"]) and not no_h["hessian"].any()
    # the pair list of the call without `pairs` is the one handed in
    free = vgicp_numpy(pose, *args)
    assert free["score"] == at["score"] and free["n_pairs"] == at["n_pairs"]


def test_newton_align_over_the_restatement_converges(pkg, side):
    """ndt_newton_align driven by vgicp_numpy from the scene's guess (0.1 m / 8.73e-3 rad off).  DIRECT1 must converge and
    end closer to the true pose than the guess in translation and rotation; the figures are printed and recorded in DESIGN
    7q, not gated: DIRECT1 2 iterations (6 evaluations), 0.0094 m / 3.14e-4 rad from the true pose; DIRECT7 5 iterations (17
    evaluations), 0.0259 m / 9.32e-4 rad (the wider neighbourhood is the less exact one: neighbouring voxels of other
    surfaces pull)."""
    from slam_sam_amd import synth
    S = side["S"]
    e_guess = synth.pose_error(side["guess"], side["truth"])
    for method in ("DIRECT1", "DIRECT7"):
        log = []
        r = vgicp_align_numpy(pkg, side["ideal"], S["cov"], S["found"], side["voxels"], side["leaves"], side["grid"], method,
                              side["guess"], log=log)
        dt, dr = synth.pose_error(r["T"], side["truth"])
        print("newton_align over the restatement, %s: converged %d, %d iterations, %d evaluations, %.4f m %.2e rad from the true pose "
              "(guess %.4f m %.2e rad)" % (method, r["converged"], r["iterations"], len(log), dt, dr, e_guess[0], e_guess[1]))
        if method == "DIRECT1":
            assert r["converged"] and 1 <= r["iterations"] < KW["max_iterations"]
            assert dt < e_guess[0] and dr < e_guess[1]


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    vp, dp, fp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float)
    want = {
        "ndt_vgicp_export_voxels": [vp, vp, dp, dp, C.c_size_t],
        "ndt_vgicp_get_info": [vp, C.POINTER(pkg.VgicpInfo)],
        "ndt_eval_derivatives_vgicp": [vp, dp, C.c_int, C.c_int, dp],
        "ndt_align_vgicp": [vp, fp, C.POINTER(pkg.Result), C.POINTER(pkg.VgicpInfo)],
    }
    for name in NEW:
        assert re.search(r"\b(?:int|int64_t)\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS
        assert list(getattr(L, name).argtypes) == want[name], name
    assert L.ndt_vgicp_export_voxels.restype is C.c_int64
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for decl in ("int64_t ndt_vgicp_export_voxels(ndt_handle* h, int32_t* count, double* mean3, double* cov6, size_t cap);",
                 "int ndt_vgicp_get_info(ndt_handle* h, ndt_vgicp_info* out);",
                 "int ndt_eval_derivatives_vgicp(ndt_handle* h, const double* poses6, int K, int compute_hessian, double* out);",
                 "int ndt_align_vgicp(ndt_handle* h, const float guess_colmajor[16], ndt_result* out, ndt_vgicp_info* info_or_null);"):
        assert decl in flat, decl
    fields = re.search(r"typedef struct ndt_vgicp_info \{(.*?)\} ndt_vgicp_info;", flat).group(1)
    assert re.findall(r"\b(n_\w+)\b", fields) == [k for k, _ in pkg.VgicpInfo._fields_]
    assert all(t is C.c_int64 for _, t in pkg.VgicpInfo._fields_) and C.sizeof(pkg.VgicpInfo) == 56
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3      # additive: no new version
    hpp = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    assert re.search(r"class VoxelizedGeneralizedIterativeClosestPoint\s*:\s*public GeneralizedIterativeClosestPoint<", hpp)
    assert "ndt_align_vgicp(" in hpp and re.search(r"\bvgicpInfo\s*\(", hpp)
    assert not os.path.exists(os.path.join(ROOT, "include", "compat", "pclomp", "vgicp_omp.h"))
    for m in ("vgicpVoxels", "vgicpInfo", "evalDerivativesVGICP", "alignVGICP"):
        fn = getattr(pkg, m)
        assert callable(fn) and fn.__code__.co_varnames[0] == "engine", m
    mk = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "Makefile")).read()
    assert "$(B)/ndt_vgicp.o" in mk


def test_argument_errors_come_before_the_handle(pkg):
    L = pkg.lib()
    pose = (C.c_double * 6)()
    words = (C.c_double * 32)()
    guess = (C.c_float * 16)()
    cnt = (C.c_int32 * 4)()
    mean = (C.c_double * 24)()
    res, info = pkg.Result(), pkg.VgicpInfo()
    info.n_voxels = 7
    # NULL handle
    assert L.ndt_vgicp_export_voxels(None, cnt, mean, mean, 2) == -1
    assert L.ndt_vgicp_get_info(None, C.byref(info)) == -1 and info.n_voxels == 7
    assert L.ndt_eval_derivatives_vgicp(None, pose, 1, 1, words) == -1
    assert L.ndt_align_vgicp(None, guess, C.byref(res), C.byref(info)) == -1 and info.n_voxels == 7
    # the argument checks come before the handle is looked at: a stand-in block of zero bytes is never read
    h = C.create_string_buffer(1 << 16)
    assert L.ndt_vgicp_get_info(h, None) == -1
    nan_pose = (C.c_double * 6)(0, 0, 0, 0, np.nan, 0)
    inf_pose = (C.c_double * 6)(np.inf, 0, 0, 0, 0, 0)
    two = (C.c_double * 12)(*([0.0] * 11 + [np.nan]))                                 # the second pose of two
    assert L.ndt_eval_derivatives_vgicp(h, None, 1, 1, words) == -1
    assert L.ndt_eval_derivatives_vgicp(h, pose, 1, 1, None) == -1
    assert L.ndt_eval_derivatives_vgicp(h, pose, 0, 1, words) == -1
    assert L.ndt_eval_derivatives_vgicp(h, pose, -3, 1, words) == -1
    for bad in (nan_pose, inf_pose):
        assert L.ndt_eval_derivatives_vgicp(h, bad, 1, 1, words) == -1
    assert L.ndt_eval_derivatives_vgicp(h, two, 2, 1, words) == -1
    assert L.ndt_align_vgicp(h, None, C.byref(res), C.byref(info)) == -1
    assert L.ndt_align_vgicp(h, guess, None, C.byref(info)) == -1
    assert bytes(h.raw) == bytes(1 << 16) and not any(words) and info.n_voxels == 7   # nothing was written


def test_python_functions_validate_before_the_library(pkg):
    ndt = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)   # no handle: nothing may reach the library
    ndt._h = None
    bad = [
        lambda: pkg.evalDerivativesVGICP(ndt, np.zeros(5)),
        lambda: pkg.evalDerivativesVGICP(ndt, np.zeros((2, 7))),
        lambda: pkg.evalDerivativesVGICP(ndt, np.full((2, 6), np.nan)),
        lambda: pkg.evalDerivativesVGICP(ndt, np.full(6, np.inf)),
        lambda: pkg.alignVGICP(ndt, np.zeros((3, 3))),
        lambda: pkg.alignVGICP(ndt, np.full((4, 4), np.nan)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d reached the library" % k)


# ---- the kernels --------------------------------------------------------------------------------------------------------
def test_vgicp_kernels_do_not_spill(tmp_path):
    """ndt_vgicp.hip for gfx950 (the figures tools/kernel_resources.py prints for `ndt_vgicp.hip k_vgicp_`): every kernel
    carries k_vgicp_, none uses scratch, and the Hessian instances of k_vgicp_eval stay within the 256 architectural VGPRs
    without borrowing accumulation registers; the figures go to profiles/vgicp_resources.txt.  Shared code is called, not
    copied."""
    path, usage = kernel_resources("ndt_vgicp.hip", tmp_path)
    assert usage and all("k_vgicp_" in k for k in usage), sorted(usage)
    kernels = {re.search(r"k_vgicp_[a-z_]+?(?=I|E)", k).group(0) for k in usage}
    assert kernels == {"k_vgicp_keys", "k_vgicp_voxels", "k_vgicp_eval"}, kernels
    assert len(usage) == 6                                                   # k_vgicp_eval: <HESSIAN, D7> four times
    lines = ["kernel resources of slam-sam_amd/csrc/ndt_vgicp.hip for gfx950 (-O3 -ffp-contract=off; tests/test_vgicp_cpu.py writes this file)",
             "%-28s %6s %6s %8s %10s %6s" % ("kernel", "VGPRs", "AGPRs", "scratch", "occupancy", "LDS")]
    for k in sorted(usage):
        u = usage[k]
        short = re.search(r"k_vgicp_[a-z_]+?(?=I|E)", k).group(0) + "".join("<%s>" % a for a in re.findall(r"IL[ib](\d+)E", k))
        args = re.search(r"k_vgicp_evalILb(\d)ELb(\d)E", k)
        if args:
            short = "k_vgicp_eval<H %s, D7 %s>" % args.groups()
        lines.append("%-28s %6d %6d %8d %10d %6d" % (short, u["VGPRs"], u.get("AGPRs", 0), u["ScratchSize"], u.get("Occupancy", 0),
                                                    u.get("LDS", 0)))
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 256, (k, u)
        if args and args.group(1) == "1":
            assert u.get("AGPRs", 0) == 0, (k, u)
    print("\n".join(lines))
    with open(os.path.join(ROOT, "profiles", "vgicp_resources.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    src = open(path).read()
    assert len(re.findall(r"__global__", src)) == len(kernels)
    # no atomics at all (the sums are sequential per leaf), no inline assembly
    assert not re.findall(r"atomic\w*\(", src) and not re.search(r"\basm\b", src)
    # the neighbour rule, the pair rule, the sort, the block row and the host driver are the shared ones
    assert '#include "ndt_neighbors_device.h"' in src and "neighbor_cells7<" in src and "neighbor_slots7<" in src and "floorf(" not in src
    assert '#include "ndt_d2d_device.h"' in src and "d2d_pair<" in src and "D2dCountWeight" in src and "d2d_words(" in src
    assert "sort_keyed(" in src and "sort_put_plan(" in src
    assert "eval_block_row<" in src and "__shfl_xor" not in src and "lane_eval_rows(" in src and "lane_align(" in src
    assert "gicp_target_ready(" in src and "gicp_source_ready(" in src and "k_gicp_" not in src
    dev = open(os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_d2d_device.h")).read()
    assert "struct D2dCountWeight" in dev and "QQ = false" in dev.split("struct D2dCountWeight")[1].split("};")[0]
    # no environment variable is read
    assert "getenv" not in src
