"""Distribution-to-distribution NDT on the device (ndt_set_source_distributions / _device, ndt_eval_derivatives_d2d,
ndt_align_d2d) against the NumPy restatement of the header's rule (test_d2d_cpu.d2d_numpy), fed with the engine's own
getLeaves(), getGridInfo() and ndt_export_source_distributions.
Scene (test_d2d_cpu.scene): hilly ground and building faces on 48 m x 48 m, 1.0 m leaf; engine A's map holds the 36 000
target points and becomes the target through setInputTargetFromMapMoments, engine B's map holds another sample of the
surfaces (30 000 points, moved by the inverse of a pose of about 0.3 m and 2 degrees) plus four voxels that test the
leaf rule, and its mapExportState is the distribution source.
Tolerances are those of tests/test_gpu_parity.py for "the same formulas in f64": score and nvtl_sum 1e-9 relative, gradient
and Hessian 1e-9 of their norms, the three counters equal; the align within 1 mm / 0.1 mrad of the CPU run of
ndt_newton_align over the restatement, in the same number of iterations."""
import os
import subprocess

import numpy as np
import pytest

from test_d2d_cpu import (ATTITUDE, KW, d2d_numpy, d2d_pairs, gauss_constants, moved_means, restatement_evaluator, scene)
from test_gpu_map_target import code_of
from test_map_state_cpu import states_equal

pytestmark = pytest.mark.gpu

ALIGN_TOL_M, ALIGN_TOL_RAD = 1e-3, 1e-4
INVALID_ARG, NO_TARGET, NO_SOURCE, UNSUPPORTED = -1, -4, -5, -9
POSE_NEAR = np.array([0.21, -0.13, 0.05, 0.012, -0.008, 0.025])            # identity attitude, near the answer
POSE_ID = np.zeros(6)
POSE_ATT = np.array([0.21, -0.13, 0.05, *ATTITUDE])
SIZES = (1, 63, 64, 65, 256, 257, None)                                      # a lone lane, the wave edge, the block edge, several blocks


def engine(pkg, **kw):
    return pkg.NormalDistributionsTransform(device_id=0, resolution=1.0, **dict(KW, **kw))


def map_of(pkg, cloud, **kw):
    ndt = engine(pkg, **kw)
    ndt.mapReset(1.0)
    ndt.mapEnableMoments()
    ndt.mapAdd(cloud)
    return ndt


def rule_voxels():
    """Four voxels far from everything (x around 60 m), each a case of the leaf rule: 2 points and 5 points (below the
    minimum count of 6), 8 coincident points (no extent: the rule's eigenvalue check rejects it) and 8 collinear points
    (the rule floors the two vanishing eigenvalues: whatever the target build makes of it, the source does too)."""
    rng = np.random.default_rng(5)
    two = np.array([60.5, 0.5, 0.5]) + rng.uniform(-0.3, 0.3, (2, 3))
    five = np.array([62.5, 0.5, 0.5]) + rng.uniform(-0.3, 0.3, (5, 3))
    same = np.tile([64.5, 0.25, 0.75], (8, 1))
    line = np.array([66.1, 0.2, 0.3]) + np.linspace(0.0, 0.7, 8)[:, None] * np.array([1.0, 0.5, 0.25])
    return np.concatenate([two, five, same, line]).astype(np.float32)


def upper6(cov):
    """xx, xy, xz, yy, yz, zz of getLeaves()' 3 x 3 covariances: the triangle a source Gaussian and the kernel's target
    leaves hold (a covariance the eigenvalue floor recomposed is symmetric only up to the last bit)"""
    return np.ascontiguousarray(np.asarray(cov)[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]])


def words_of(pkg, ndt, poses, hessian=True):
    """the packed words of a D2D evaluation, as bits"""
    return pkg.evalDerivativesD2D(ndt, poses, compute_hessian=hessian, raw=True).view(np.uint64).copy()


def assert_face_clear(pose, mean, leaf=1.0):
    """the precondition on the INPUTS: no moved mean within 1e-6 of a voxel face (there the f32 classification of the kernel
    and of the restatement would have to agree on the last bit of an f64 sum); if it fails, pick another seed or pose"""
    m = moved_means(pose, mean) / leaf
    d = np.abs(m - np.round(m)) * leaf
    assert d.min() >= 1e-6, "a moved mean lies %.2e from a voxel face at pose %s" % (d.min(), pose)


def assert_matches(got, want, tol=1e-9):
    assert got["n_pairs"] == want["n_pairs"] and got["n_with_neighbors"] == want["n_with_neighbors"]
    assert got["score"] == pytest.approx(want["score"], rel=tol, abs=1e-12)
    assert got["nvtl_sum"] == pytest.approx(want["nvtl_sum"], rel=tol, abs=1e-12)
    gn, hn = np.linalg.norm(want["gradient"]), np.linalg.norm(want["hessian"])
    assert np.linalg.norm(got["gradient"] - want["gradient"]) <= tol * gn + 1e-12
    assert np.linalg.norm(got["hessian"] - want["hessian"]) <= tol * hn + 1e-12


@pytest.fixture(scope="module")
def rig(pkg):
    from slam_sam_amd import synth
    s = scene()
    A = map_of(pkg, s["target"])
    A.setInputTargetFromMapMoments()
    A.setInputSource(s["source"][::4])                                      # a point source beside the distribution source
    cloud_b = np.concatenate([s["source"], rule_voxels()])
    B = map_of(pkg, cloud_b)
    state = B.mapExportState()
    # the same submap turned back by the attitude of POSE_ATT, so that POSE_ATT puts it on the target again
    back = np.linalg.inv(synth.pose_matrix(0, 0, 0, *ATTITUDE))
    state_att = map_of(pkg, synth.transform(back, s["source"]).astype(np.float32)).mapExportState()
    d1, d2 = gauss_constants(pkg)
    return dict(A=A, B=B, state=state, state_att=state_att, tgt=A.getLeaves(), grid=A.getGridInfo(), d1=d1, d2=d2,
                truth=s["truth"], cloud_b=cloud_b)


def set_source(pkg, ndt, state, n=None, accepted_only=None):
    count, mom = state["count"], state["moments"]
    if accepted_only is not None:
        count, mom = count[accepted_only], mom[accepted_only]
    pkg.setSourceDistributions(ndt, count=count[:n], moments=mom[:n])
    return pkg.getSourceDistributions(ndt)


# ---- 1. the source Gaussians are the target build's leaves --------------------------------------------------------------
def test_source_gaussians_are_the_leaves_of_the_same_moments(pkg, rig):
    A, B, state = rig["A"], rig["B"], rig["state"]
    B.setInputTargetFromMapMoments()
    L = B.getLeaves()
    n_rec, n_acc = pkg.setSourceDistributions(A, state)
    assert n_rec == len(state["count"]) and n_acc == len(L["count"]) and 2000 < n_acc < n_rec
    G = pkg.getSourceDistributions(A)
    assert np.array_equal(G["count"], L["count"])
    assert np.array_equal(G["mean"].view(np.uint64), L["mean"].view(np.uint64))                  # bit for bit
    assert np.array_equal(G["cov6"].view(np.uint64), upper6(L["cov"]).view(np.uint64))
    assert np.all(np.diff(G["record_index"]) > 0)                                                # input order
    assert np.array_equal(state["count"][G["record_index"]], G["count"])
    # the four rule voxels: below the minimum count and without extent -> rejected and absent
    x = state["moments"][:, 0] / state["count"]
    rec = {name: int(np.nonzero((x > lo) & (x < lo + 1))[0][0]) for name, lo in (("two", 60), ("five", 62), ("same", 64), ("line", 66))}
    assert [int(state["count"][rec[k]]) for k in ("two", "five", "same", "line")] == [2, 5, 8, 8]
    for k in ("two", "five", "same"):
        assert rec[k] not in G["record_index"], k
    rejected = np.setdiff1d(np.arange(n_rec), G["record_index"])
    assert len(rejected) == n_rec - n_acc and (state["count"][rejected] < 6).sum() >= 2
    # (the collinear voxel follows the build: in the source exactly when it is a leaf of the target made of these moments)
    line_is_leaf = bool(np.any(np.all(np.abs(L["mean"] - state["moments"][rec["line"], :3] / 8) < 1e-9, axis=1)))
    assert (rec["line"] in G["record_index"]) == line_is_leaf
    print("source: %d records, %d accepted; collinear voxel accepted: %s" % (n_rec, n_acc, line_is_leaf))


def test_a_changed_leaf_rule_rederives_the_gaussians(pkg, rig):
    """ndt_set_params keeps the records: with min_points_per_voxel = 12 the Gaussians are those of a target rebuilt from
    the same moments under that rule, without the source being set again"""
    s = scene()
    B = map_of(pkg, s["source"][:12000])
    st = B.mapExportState()
    A = engine(pkg)
    n_rec, n6 = pkg.setSourceDistributions(A, st)
    A.setMinPointPerVoxel(12)
    B.setMinPointPerVoxel(12)
    B.setInputTargetFromMapMoments()
    L = B.getLeaves()
    assert pkg.sourceDistributionsInfo(A) == (n_rec, len(L["count"])) and 0 < len(L["count"]) < n6
    G = pkg.getSourceDistributions(A)
    assert G["count"].min() >= 12 and np.array_equal(G["count"], L["count"])
    assert np.array_equal(G["mean"].view(np.uint64), L["mean"].view(np.uint64))
    assert np.array_equal(G["cov6"].view(np.uint64), upper6(L["cov"]).view(np.uint64))
    assert pkg.setSourceDistributions(A, count=np.zeros(0), moments=np.zeros((0, 9))) == (0, 0)  # n = 0 clears
    assert len(pkg.getSourceDistributions(A)["count"]) == 0


# ---- 2. the evaluation is the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT1"])
@pytest.mark.parametrize("which", ["near", "attitude"])
def test_evaluation_equals_the_restatement(pkg, rig, method, which):
    A = rig["A"]
    A.setNeighborhoodSearchMethod(pkg.DIRECT7 if method == "DIRECT7" else pkg.DIRECT1)
    state, pose = (rig["state"], POSE_NEAR) if which == "near" else (rig["state_att"], POSE_ATT)
    try:
        full = set_source(pkg, A, state)
        accepted = full["record_index"]
        cases = [(n, None) for n in SIZES] + [(n, accepted) for n in SIZES[:-1]]   # records as exported; exactly n Gaussians
        for n, only in cases:
            src = set_source(pkg, A, state, n, only)
            if only is not None:
                assert len(src["count"]) == n
            if len(src["count"]) == 0:                                             # (a prefix none of whose records passes)
                assert code_of(pkg, pkg.evalDerivativesD2D, A, pose) == NO_SOURCE
                continue
            assert_face_clear(pose, src["mean"])
            want = d2d_numpy(pose, src, rig["tgt"], rig["grid"], rig["d1"], rig["d2"], method)
            got = pkg.evalDerivativesD2D(A, pose)[0]
            assert_matches(got, want)
            if n is None:
                assert want["n_pairs"] > (5000 if method == "DIRECT7" else 1500)
                print("%s %s: %d Gaussians, %d pairs, score %.6f" % (method, which, len(src["count"]), want["n_pairs"], want["score"]))
    finally:
        A.setNeighborhoodSearchMethod(pkg.DIRECT7)


def test_identity_pose_outside_and_straddling(pkg, rig):
    A = rig["A"]
    src = set_source(pkg, A, rig["state"])
    ext = (rig["grid"]["max_b"][0] - rig["grid"]["min_b"][0] + 1) * 1.0
    poses = {"identity": POSE_ID, "outside": np.array([1000.0, 0, 0, 0, 0, 0]),
             "straddle": np.array([ext / 2 + 0.37, 0.21, 0.05, 0.0, 0.0, 0.01])}
    for name, pose in poses.items():
        assert_face_clear(pose, src["mean"])
        want = d2d_numpy(pose, src, rig["tgt"], rig["grid"], rig["d1"], rig["d2"])
        got = pkg.evalDerivativesD2D(A, pose)[0]
        assert_matches(got, want)
        if name == "outside":
            assert want["n_pairs"] == 0 and not words_of(pkg, A, pose).any()        # zero pairs: every word is +0
        if name == "straddle":
            m = moved_means(pose, src["mean"])[:, 0]
            hi = (rig["grid"]["max_b"][0] + 1) * 1.0
            assert (m < hi).sum() > 200 and (m >= hi).sum() > 200 and 0 < want["n_with_neighbors"] < (m < hi + 1).sum()


# ---- 3. bits ------------------------------------------------------------------------------------------------------------
def test_bit_identity(pkg, rig, hipmem):
    A, state = rig["A"], rig["state"]
    set_source(pkg, A, state)
    poses = np.stack([POSE_NEAR, POSE_ID, POSE_NEAR + [0.1, 0.05, -0.02, 0.004, 0.003, -0.01]])
    w3 = words_of(pkg, A, poses)
    assert np.array_equal(w3, words_of(pkg, A, poses))                               # two calls
    for k in range(3):                                                               # a pose alone = the pose in a batch
        assert np.array_equal(words_of(pkg, A, poses[k])[0], w3[k]), k
    assert len({w.tobytes() for w in w3}) == 3
    # without the Hessian: its words are zero, score / gradient / counters are the SAME BITS (one code path for both
    # instantiations, no contraction)
    w0 = words_of(pkg, A, poses, hessian=False)
    assert not w0[:, 7:28].any() and w3[:, 7:28].any()
    assert np.array_equal(w0[:, :7], w3[:, :7]) and np.array_equal(w0[:, 28:], w3[:, 28:])
    # the device setter gives the bits of the host setter
    G = pkg.getSourceDistributions(A)
    d_count = hipmem.upload(np.ascontiguousarray(state["count"], np.int32))
    d_mom = hipmem.upload(np.ascontiguousarray(state["moments"], np.float64))
    assert pkg.setSourceDistributionsDevice(A, d_count, d_mom, len(state["count"])) == (len(state["count"]), len(G["count"]))
    G2 = pkg.getSourceDistributions(A)
    for k in ("mean", "cov6", "count", "record_index"):
        assert np.array_equal(G[k], G2[k]) and G[k].tobytes() == G2[k].tobytes(), k
    assert np.array_equal(words_of(pkg, A, poses), w3)


def test_refusals_keep_the_previous_source(pkg, rig, hipmem):
    A, state = rig["A"], rig["state"]
    set_source(pkg, A, state)
    before = words_of(pkg, A, POSE_NEAR)
    info = pkg.sourceDistributionsInfo(A)
    L = pkg.lib()
    cnt = np.ascontiguousarray(state["count"][:300], np.int32)
    mom = np.ascontiguousarray(state["moments"][:300], np.float64)
    zero = cnt.copy()
    zero[123] = 0
    nan = mom.copy()
    nan[250, 4] = np.nan
    inf = mom.copy()
    inf[7, 0] = np.inf
    assert L.ndt_set_source_distributions(A._h, None, mom.ctypes.data, 300) == INVALID_ARG
    assert L.ndt_set_source_distributions(A._h, cnt.ctypes.data, None, 300) == INVALID_ARG
    assert L.ndt_set_source_distributions(A._h, zero.ctypes.data, mom.ctypes.data, 300) == INVALID_ARG
    assert L.ndt_set_source_distributions(A._h, cnt.ctypes.data, nan.ctypes.data, 300) == INVALID_ARG
    assert L.ndt_set_source_distributions(A._h, cnt.ctypes.data, inf.ctypes.data, 300) == INVALID_ARG
    d_cnt, d_mom, d_zero, d_nan = (hipmem.upload(a) for a in (cnt, mom, zero, nan))
    assert L.ndt_set_source_distributions_device(A._h, None, d_mom, 300) == INVALID_ARG
    assert L.ndt_set_source_distributions_device(A._h, d_zero, d_mom, 300) == INVALID_ARG
    assert L.ndt_set_source_distributions_device(A._h, d_cnt, d_nan, 300) == INVALID_ARG
    assert L.ndt_export_source_distributions(A._h, None, None, None, None, 3) == INVALID_ARG     # cap below the count
    assert pkg.sourceDistributionsInfo(A) == info
    assert np.array_equal(words_of(pkg, A, POSE_NEAR), before)                       # the previous source evaluates as before


def test_unsupported_configurations(pkg, rig):
    A = rig["A"]
    set_source(pkg, A, rig["state"])
    before = words_of(pkg, A, POSE_NEAR)
    try:
        for method in (pkg.KDTREE, pkg.DIRECT26):
            A.setNeighborhoodSearchMethod(method)
            assert code_of(pkg, pkg.evalDerivativesD2D, A, POSE_NEAR) == UNSUPPORTED
            assert code_of(pkg, pkg.alignDistributions, A) == UNSUPPORTED
    finally:
        A.setNeighborhoodSearchMethod(pkg.DIRECT7)
    assert np.array_equal(words_of(pkg, A, POSE_NEAR), before)
    s = scene()
    U = engine(pkg)                                                                  # a multi-grid union target
    U.addTarget(s["target"][:18000], 0)
    U.addTarget(s["target"][18000:], 1)
    U.createVoxelKdtree()
    pkg.setSourceDistributions(U, rig["state"])
    assert code_of(pkg, pkg.evalDerivativesD2D, U, POSE_NEAR) == UNSUPPORTED
    H = map_of(pkg, s["target"])                                                     # a hook reducer
    H.setInputTargetFromMapMoments()
    pkg.setSourceDistributions(H, rig["state"])
    assert pkg.evalDerivativesD2D(H, POSE_NEAR)[0]["n_pairs"] > 0
    H.commInitHook(lambda _ctx, _w, _n: 0, 0, 1)
    assert code_of(pkg, pkg.evalDerivativesD2D, H, POSE_NEAR) == UNSUPPORTED
    assert code_of(pkg, pkg.alignDistributions, H) == UNSUPPORTED
    # no target, no distribution source: the guess comes back
    N = engine(pkg)
    assert code_of(pkg, pkg.evalDerivativesD2D, N, POSE_NEAR) == NO_TARGET
    res = pkg.Result()
    g = np.ascontiguousarray(np.eye(4, dtype=np.float32).T).ravel()
    g[12] = 0.5
    import ctypes as C
    assert pkg.lib().ndt_align_d2d(N._h, g.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res)) == NO_TARGET
    assert res.converged == 0 and list(res.final_transformation) == list(g)
    T2 = map_of(pkg, s["target"])
    T2.setInputTargetFromMapMoments()
    assert pkg.lib().ndt_align_d2d(T2._h, g.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res)) == NO_SOURCE
    assert res.converged == 0 and list(res.final_transformation) == list(g)
    pkg.setSourceDistributions(T2, count=rig["state"]["count"][:1] * 0 + 2, moments=rig["state"]["moments"][:1])   # one record, rejected
    assert pkg.sourceDistributionsInfo(T2) == (1, 0)
    assert pkg.lib().ndt_align_d2d(T2._h, g.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res)) == NO_SOURCE


# ---- 4. the align -------------------------------------------------------------------------------------------------------
def test_align_follows_newton_over_the_restatement(pkg, rig):
    from slam_sam_amd import synth
    A = rig["A"]
    src = set_source(pkg, A, rig["state"])
    guess = np.eye(4)
    T0 = A.align(guess)                                                              # the point-to-distribution align of the handle
    r0, h0 = A.getResult(), A.getIterationHistory()
    T, r = pkg.alignDistributions(A, guess)
    ev = restatement_evaluator(pkg, src, rig["tgt"], rig["grid"], rig["d1"], rig["d2"])
    ref = pkg.newton_align(pkg.default_params(resolution=1.0, **KW), len(src["count"]), guess, ev)
    dt, dr = synth.pose_error(T, ref["T"])
    gt = synth.pose_error(T, rig["truth"])
    print("alignDistributions: %d iterations (restatement %d), %.2e m %.2e rad from it, %.4f m %.2e rad from the true pose"
          % (r["iterations"], ref["iterations"], dt, dr, gt[0], gt[1]))
    assert r["converged"] and ref["converged"]
    assert dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD
    assert r["iterations"] == ref["iterations"]
    assert gt[0] < 0.05 and gt[1] < 0.005
    # the handle's own align is left alone: history unchanged, the same bits again
    h1 = A.getIterationHistory()
    assert all(np.array_equal(a, b) for a, b in zip(h0, h1)) and len(h0[1]) > 1
    T1 = A.align(guess)
    r1 = A.getResult()
    assert np.array_equal(T1.view(np.uint64), T0.view(np.uint64))
    for k in ("pose", "hessian"):
        assert np.array_equal(np.asarray(r1[k]).view(np.uint64), np.asarray(r0[k]).view(np.uint64)), k
    assert (r1["iterations"], r1["n_evaluations"], r1["transform_probability"], r1["nvtl"]) == \
           (r0["iterations"], r0["n_evaluations"], r0["transform_probability"], r0["nvtl"])
    assert all(np.array_equal(a, b) for a, b in zip(h0, A.getIterationHistory()))


# ---- 5. submap -> pose -> posed import, on the device --------------------------------------------------------------------
def test_the_chain_closes_on_the_device(pkg, rig, hipmem):
    A, B, state = rig["A"], rig["B"], rig["state"]
    cap = B.mapInfo()["n_voxels"]
    d_ijk = hipmem.upload(np.zeros((cap, 3), np.int32))
    d_cnt = hipmem.upload(np.zeros(cap, np.int32))
    d_sums = hipmem.upload(np.zeros((cap, 4), np.float32))
    d_mom = hipmem.upload(np.zeros((cap, 9), np.float64))
    m = B.mapExportStateDevice(d_ijk, d_cnt, d_sums, d_mom, cap)
    assert m == len(state["count"]) == cap
    n_rec, n_acc = pkg.setSourceDistributionsDevice(A, d_cnt, d_mom, m)
    assert n_rec == m and n_acc > 2000
    T, r = pkg.alignDistributions(A)
    assert r["converged"]
    host = map_of(pkg, scene()["target"])                                            # the same map, the records through the host
    before = A.mapInfo()
    pkg.mapImportStatePosedDevice(A, 1.0, d_ijk, d_cnt, d_sums, d_mom, m, T)
    pkg.mapImportStatePosed(host, state, T)
    a, h = A.mapInfo(), host.mapInfo()
    assert a["n_voxels"] == h["n_voxels"] > before["n_voxels"]
    assert a["n_points"] == h["n_points"] == before["n_points"] + int(state["count"].sum())
    assert states_equal(A.mapExportState(), host.mapExportState())


# ---- 6. the C++ adapter ---------------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, tmp_path):
    """tests/cpp/test_d2d.cpp against the API mocks, built with the g++ line tests/cpp/Makefile uses for them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "tests", "cpp")
    exe = str(tmp_path / "test_d2d")
    lib = os.path.join(root, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(root, "include", "compat"), "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(d, "test_d2d.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "d2d: PASS" in p.stdout
