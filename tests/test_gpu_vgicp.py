"""Voxelised GICP on the device (ndt_vgicp_export_voxels, ndt_vgicp_get_info, ndt_eval_derivatives_vgicp, ndt_align_vgicp)
against the NumPy restatement of the header's rule (tests/test_vgicp_cpu.py): the voxel table bit for bit when the
restatement is fed the engine's own point covariances, getLeaves() and getGridInfo(); the evaluation against vgicp_numpy fed
the engine's exported covariances and table, with the tolerances of tests/test_gpu_d2d.py; the align against
ndt_newton_align over the restatement on the CPU, within the continuous-time test's bounds.
Scene (test_ct_cpu.scene): 9 000 target points and the rigid 4 500-point scan, from the CT test's guess offset."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_ct_cpu import ALIGN_TOL_M, ALIGN_TOL_RAD, scene
from test_d2d_cpu import ATTITUDE, classify
from test_gicp_cpu import MIN_NEIGHBOURS, SIZES
from test_gpu_d2d import assert_matches
from test_gpu_gicp import POSE_GENERAL, bits, defaults, engine, pairs_source, same_bits
from test_gpu_map_target import code_of
from test_vgicp_cpu import vgicp_align_numpy, vgicp_numpy, vgicp_voxels_numpy

pytestmark = pytest.mark.gpu

INVALID_ARG, NO_TARGET, NO_SOURCE, UNSUPPORTED = -1, -4, -5, -9
POSE_ATT = np.array([*POSE_GENERAL[:3], *ATTITUDE])
CAP = 0.8                                              # the finite max_neighbour_distance of the table test
CUBE = np.array([40.5, 0.5, 0.5])                      # centre of a voxel far from the scene
LONE = np.array([60.25, 0.25, 0.375], np.float32)


def table_target():
    """The scene's target and, at fixed places behind it (indices n .. n + 10): a point with a NaN coordinate, a lone point
    60 m away (one neighbour within CAP: no covariance), a ground point moved exactly onto a voxel face, and the eight
    corners of a cube of edge 0.9 m inside one voxel far from everything -- a leaf by the leaf rule, but no corner has a
    second point within CAP, so none has a covariance: N = 0."""
    t = scene()["target"]
    nan = t[10].copy()
    nan[2] = np.nan
    face = t[20].copy()
    face[0] = np.round(face[0])                                               # exactly on the face x = integer
    corners = CUBE + 0.45 * np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], np.float64)
    return np.concatenate([t, nan[None], LONE[None], face[None], corners.astype(np.float32)]).astype(np.float32)


def restated_table(pkg, ndt, target):
    """vgicp_voxels_numpy fed what the engine itself exports"""
    cov = pkg.gicpCovariances(ndt, "target")["cov"]
    _, found = pkg.gicpNeighbours(ndt, "target")
    return vgicp_voxels_numpy(target, cov, found, ndt.getLeaves(), ndt.getGridInfo()), found


def words_of(pkg, ndt, poses, hessian=True):
    return pkg.evalDerivativesVGICP(ndt, poses, compute_hessian=hessian, raw=True).view(np.uint64).copy()


@pytest.fixture(scope="module")
def rig(pkg):
    s = scene()
    A = engine(pkg)
    A.setInputTarget(s["target"])
    A.setInputSource(s["ideal"])
    defaults(pkg, A)
    return dict(s, A=A, voxels=pkg.vgicpVoxels(A), leaves=A.getLeaves(), grid=A.getGridInfo())


# ---- 1. the voxel table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resolution,min_points", [(1.0, None), (0.5, None), (1.0, 3)], ids=["res1", "res05", "min3"])
def test_voxel_table_equals_the_restatement(pkg, resolution, min_points):
    tgt = table_target()
    n0 = len(scene()["target"])
    kw = dict(resolution=resolution)
    if min_points is not None:
        kw["min_points_per_voxel"] = min_points
    ndt = engine(pkg, **kw)
    ndt.setInputTarget(tgt)
    defaults(pkg, ndt, max_neighbour_distance=CAP)
    got, info = pkg.vgicpVoxels(ndt), pkg.vgicpInfo(ndt)
    want, found = restated_table(pkg, ndt, tgt)
    leaves = ndt.getLeaves()
    L = len(leaves["cell"])
    assert got["count"].shape == (L,) and got["mean"].shape == (L, 3) and got["cov6"].shape == (L, 6)
    assert np.array_equal(got["count"], want["count"])
    assert same_bits(got["mean"], want["mean"]) and same_bits(got["cov6"], want["cov6"])
    # (the restatement on the oracle's grid: 780 leaves / 6 928 points at 1 m, 59 / 383 at 0.5 m, 1 145 / 8 462 from 3 points on)
    assert info["n_leaves"] == L and info["n_voxels"] == (want["count"] >= 1).sum() > (500 if resolution == 1.0 else 30)
    assert info["n_target_points_in_voxels"] == want["n_target_points_in_voxels"] == want["count"].sum() > (0.5 * n0 if resolution == 1.0 else 200)
    assert info["n_target_without_covariance"] == (found < MIN_NEIGHBOURS).sum()
    assert info["n_pairs"] == 0 and info["n_source_with_pairs"] == 0 and info["n_source_without_covariance"] == 0
    # the special points: none of them has a covariance except the one on the face, which counts where the f32
    # classification puts it
    assert (found[n0:n0 + 2] < MIN_NEIGHBOURS).all() and (found[n0 + 3:] == 1).all() and found[n0 + 2] >= MIN_NEIGHBOURS
    cells = np.asarray(leaves["cell"], np.int64)
    face_cell = classify(tgt[n0 + 2:n0 + 3], ndt.getGridInfo())[0]
    assert face_cell >= 0 and tgt[n0 + 2, 0] == np.round(tgt[n0 + 2, 0])
    if resolution == 1.0:
        # the cube's voxel is a leaf (8 points, full rank) whose points all lack a covariance: a NaN row with N = 0
        cube_cell = classify(CUBE[None].astype(np.float32), ndt.getGridInfo())[0]
        row = int(np.searchsorted(cells, cube_cell))
        assert cells[row] == cube_cell and leaves["count"][row] == 8
        assert got["count"][row] == 0 and np.isnan(got["mean"][row]).all() and np.isnan(got["cov6"][row]).all()
        assert (got["count"] == 0).sum() >= 1 and info["n_voxels"] < L
        assert face_cell in cells                                             # the face point's cell is a leaf
    # leaves hold at least as many points as contribute (a point without a covariance is in the leaf, not in the voxel)
    assert (got["count"] <= leaves["count"]).all()
    # the same bits from a second derivation
    pkg.gicpSetParams(ndt, k_neighbours=19)
    pkg.gicpSetParams(ndt, k_neighbours=20)
    again = pkg.vgicpVoxels(ndt)
    assert np.array_equal(again["count"], got["count"]) and same_bits(again["mean"], got["mean"]) and same_bits(again["cov6"], got["cov6"])


# ---- 2. the evaluation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_evaluation_equals_the_restatement(pkg, rig, n):
    from slam_sam_amd import synth
    A, voxels, leaves, grid = rig["A"], rig["voxels"], rig["leaves"], rig["grid"]
    defaults(pkg, A)
    back = np.linalg.inv(synth.pose_matrix(0, 0, 0, *ATTITUDE))
    try:
        for base in (POSE_GENERAL, POSE_ATT):
            src = pairs_source(n)
            if base is POSE_ATT:
                # the scan turned back, so that the pose puts it on the target; the special points stay where pairs_source
                # places them (turned as well, the far-off one would stretch the bounding box of the source's point index
                # to 2e8 cells of 1 m, every one of which the neighbour search of a cloud of fewer than k points visits)
                special = src.copy()
                src = synth.transform(back, scene()["ideal"][:n]).astype(np.float32)
                if n >= 19:
                    src[5:9] = special[5:9]
            A.setInputSource(src)
            if n < MIN_NEIGHBOURS:                                            # three points: none has a covariance
                assert code_of(pkg, pkg.evalDerivativesVGICP, A, base) == NO_SOURCE
                continue
            sc = pkg.gicpCovariances(A, "source")["cov"]
            _, sfound = pkg.gicpNeighbours(A, "source")
            if n >= 19:
                assert sfound[8] == 0 and np.isnan(sc[8]).all() and sfound[7] >= MIN_NEIGHBOURS   # the NaN point, the far-off point
            poses = base[None, :] + np.random.default_rng(n).uniform(-0.02, 0.02, (8, 6))
            poses[0] = base
            for method in ("DIRECT1", "DIRECT7"):
                A.setNeighborhoodSearchMethod(pkg.DIRECT7 if method == "DIRECT7" else pkg.DIRECT1)
                got = pkg.evalDerivativesVGICP(A, poses)
                for k in (0, 3):
                    want = vgicp_numpy(poses[k], src, sc, sfound, voxels, leaves, grid, method)
                    assert_matches(got[k], want)
                    assert got[k]["nvtl_sum"] == got[k]["score"]
                if n >= 63:
                    assert got[0]["n_pairs"] >= got[0]["n_with_neighbors"] > 0.3 * n and got[0]["score"] < 0
                    assert got[0]["n_with_neighbors"] <= n - 4                # the three points far from the target, the NaN point
                # gradient-only: the Hessian call's score and gradient, zero Hessian words
                w_h, w_g = words_of(pkg, A, poses), words_of(pkg, A, poses, hessian=False)
                assert np.array_equal(w_h[:, :7], w_g[:, :7]) and not w_g[:, 7:28].any() and np.array_equal(w_h[:, 28:], w_g[:, 28:])
                assert_matches(pkg.evalDerivativesVGICP(A, poses[3], compute_hessian=False)[0],
                               vgicp_numpy(poses[3], src, sc, sfound, voxels, leaves, grid, method, hessian=False))
                # the same bits every time, and a pose in a batch the bits it gets alone
                assert np.array_equal(words_of(pkg, A, poses), w_h)
                for k in range(8):
                    assert np.array_equal(words_of(pkg, A, poses[k])[0], w_h[k]), k
    finally:
        A.setNeighborhoodSearchMethod(pkg.DIRECT7)
        A.setInputSource(rig["ideal"])


# ---- 3. the align -----------------------------------------------------------------------------------------------------------
def test_align_follows_the_loop_over_the_restatement(pkg, rig):
    """Under DIRECT1 the engine's align follows ndt_newton_align over the restatement; under DIRECT7 it must converge and
    end closer to the true pose than the guess (the wider neighbourhood is the less exact one).  The distances from the true
    pose and from alignGICP's result are printed and recorded in DESIGN 7q, not gated."""
    from slam_sam_amd import synth
    A = rig["A"]
    defaults(pkg, A)
    A.setInputSource(rig["ideal"])
    sc = pkg.gicpCovariances(A, "source")["cov"]
    _, sfound = pkg.gicpNeighbours(A, "source")
    e_guess = synth.pose_error(rig["guess"], rig["truth"])
    Tg, _ = pkg.alignGICP(A, rig["guess"])
    try:
        for method in ("DIRECT1", "DIRECT7"):
            A.setNeighborhoodSearchMethod(pkg.DIRECT7 if method == "DIRECT7" else pkg.DIRECT1)
            T, r = pkg.alignVGICP(A, rig["guess"])
            info = r["vgicp"]
            e, eg = synth.pose_error(T, rig["truth"]), synth.pose_error(T, Tg)
            print("alignVGICP %s: %d iterations, %d evaluations, %d pairs of %d points; %.5f m %.2e rad from the true pose (guess %.5f m "
                  "%.2e rad), %.5f m %.2e rad from alignGICP's result"
                  % (method, r["iterations"], r["n_evaluations"], info["n_pairs"], info["n_source_with_pairs"], e[0], e[1],
                     e_guess[0], e_guess[1], eg[0], eg[1]))
            assert r["converged"] and e[0] < e_guess[0] and e[1] < e_guess[1]
            assert info["n_voxels"] == (rig["voxels"]["count"] >= 1).sum() and info["n_leaves"] == len(rig["leaves"]["cell"])
            assert info["n_target_points_in_voxels"] == rig["voxels"]["count"].sum()
            assert info["n_pairs"] >= info["n_source_with_pairs"] > 0.5 * len(rig["ideal"])
            assert info["n_source_without_covariance"] == 0 and info["n_target_without_covariance"] == 0
            T2, r2 = pkg.alignVGICP(A, rig["guess"])
            assert np.array_equal(T2, T) and np.array_equal(r2["pose"], r["pose"]) and r2["vgicp"] == info   # the same bits every time
            if method == "DIRECT1":
                ref = vgicp_align_numpy(pkg, rig["ideal"], sc, sfound, rig["voxels"], rig["leaves"], rig["grid"], method, rig["guess"])
                dt, dr = synth.pose_error(T, ref["T"])
                print("    the restatement: %d iterations; %.2e m %.2e rad between the two" % (ref["iterations"], dt, dr))
                assert ref["converged"] and dt < ALIGN_TOL_M and dr < ALIGN_TOL_RAD
                assert abs(r["iterations"] - ref["iterations"]) <= 1
                last = vgicp_numpy(r["pose"], rig["ideal"], sc, sfound, rig["voxels"], rig["leaves"], rig["grid"], method)
                assert 0 < info["n_pairs"] and abs(info["n_pairs"] - last["n_pairs"]) <= 0.02 * last["n_pairs"]
    finally:
        A.setNeighborhoodSearchMethod(pkg.DIRECT7)


# ---- 4. state ---------------------------------------------------------------------------------------------------------------
def test_other_aligns_do_not_see_it(pkg, rig):
    """align, alignGICP, getFitnessScore and the frozen GICP pairs give the same bits before and after alignVGICP, and on
    an engine that never ran it"""
    s = rig
    A, B = engine(pkg), engine(pkg)
    for ndt in (A, B):
        ndt.setInputTarget(s["target"])
        ndt.setInputSource(s["ideal"])

    def snapshot(ndt):
        T = ndt.align(s["guess"])
        r = ndt.getResult()
        f = ndt.getFitnessScore()
        Tg, rg = pkg.alignGICP(ndt, s["guess"])
        n_pairs = pkg.gicpPair(ndt, rg["pose"])
        idx, d2 = pkg.gicpPairs(ndt)
        w = pkg.evalDerivativesGICP(ndt, rg["pose"], raw=True).view(np.uint64).copy()
        return dict(T=T, pose=r["pose"], it=r["iterations"], score=r["score"], H=r["hessian"], f=f, Tg=Tg, pg=rg["pose"],
                    gicp=rg["gicp"], n_pairs=n_pairs, idx=idx, d2=bits(d2), w=w)

    def same(a, b):
        return all(np.array_equal(a[k], b[k]) for k in ("T", "pose", "H", "Tg", "pg", "idx", "d2", "w")) and \
            all(a[k] == b[k] for k in ("it", "score", "f", "gicp", "n_pairs"))

    before = snapshot(A)
    idx0, d20 = pkg.gicpPairs(A)
    Tv, rv = pkg.alignVGICP(A, s["guess"])
    pkg.evalDerivativesVGICP(A, rv["pose"])
    idx1, d21 = pkg.gicpPairs(A)                                              # the frozen pairs are still there, untouched
    assert np.array_equal(idx0, idx1) and np.array_equal(bits(d20), bits(d21)) and (idx1 >= 0).sum() == before["n_pairs"]
    assert np.array_equal(pkg.evalDerivativesGICP(A, before["pg"], raw=True).view(np.uint64), before["w"])
    assert np.array_equal(A.getResult()["pose"], before["pose"])               # getResult() keeps reporting the last align()
    after = snapshot(A)
    assert same(before, after)
    assert same(before, snapshot(B))
    assert not np.array_equal(Tv, before["T"]) and rv["converged"]


def test_table_and_source_follow_their_inputs(pkg, rig):
    s = rig
    A = engine(pkg)
    A.setInputTarget(s["target"])
    A.setInputSource(s["ideal"])
    defaults(pkg, A)
    base_info, base = pkg.vgicpInfo(A), pkg.vgicpVoxels(A)
    assert base_info["n_source_without_covariance"] == 0 and base_info["n_voxels"] == (rig["voxels"]["count"] >= 1).sum()
    assert np.array_equal(base["count"], rig["voxels"]["count"]) and same_bits(base["cov6"], rig["voxels"]["cov6"])

    def consistent(ndt, target):
        got, info = pkg.vgicpVoxels(ndt), pkg.vgicpInfo(ndt)
        want, _ = restated_table(pkg, ndt, target)
        assert np.array_equal(got["count"], want["count"]) and same_bits(got["mean"], want["mean"]) and same_bits(got["cov6"], want["cov6"])
        assert info["n_leaves"] == len(got["count"]) and info["n_target_points_in_voxels"] == got["count"].sum()
        return got, info

    # a changed k_neighbours: other covariances in the same voxels
    pkg.gicpSetParams(A, k_neighbours=10)
    got, info = consistent(A, s["target"])
    assert np.array_equal(got["count"], base["count"]) and not same_bits(got["cov6"], base["cov6"]) and same_bits(got["mean"], base["mean"])
    defaults(pkg, A)
    got, _ = consistent(A, s["target"])
    assert same_bits(got["cov6"], base["cov6"])
    # a changed resolution: other voxels
    A.setResolution(2.0)
    got, info = consistent(A, s["target"])
    assert info["n_leaves"] < base_info["n_leaves"] and info["n_target_points_in_voxels"] > base_info["n_target_points_in_voxels"]
    A.setResolution(1.0)
    got, info = consistent(A, s["target"])
    assert info == base_info and same_bits(got["cov6"], base["cov6"])
    # a new target
    A.setInputTarget(s["target"][:6000])
    got, info = consistent(A, s["target"][:6000])
    assert 0 < info["n_target_points_in_voxels"] < base_info["n_target_points_in_voxels"] and info["n_leaves"] != base_info["n_leaves"]
    A.setInputTarget(s["target"])
    # a new source is picked up
    pose = POSE_GENERAL
    full = pkg.evalDerivativesVGICP(A, pose)[0]
    A.setInputSource(s["ideal"][:2000])
    part = pkg.evalDerivativesVGICP(A, pose)[0]
    sc = pkg.gicpCovariances(A, "source")["cov"]
    _, sfound = pkg.gicpNeighbours(A, "source")
    assert len(sfound) == 2000 and 0 < part["n_with_neighbors"] < full["n_with_neighbors"] and part["n_with_neighbors"] <= 2000
    assert_matches(part, vgicp_numpy(pose, s["ideal"][:2000], sc, sfound, pkg.vgicpVoxels(A), A.getLeaves(), A.getGridInfo(), "DIRECT7"))
    _, r = pkg.alignVGICP(A, s["guess"])
    assert r["converged"] and r["vgicp"]["n_source_with_pairs"] <= 2000


def test_errors(pkg, rig, hipmem):
    s = rig
    L = pkg.lib()
    C0 = engine(pkg)
    guess_bits = np.asarray(s["guess"], np.float32)

    def align_leaves_the_guess(ndt, code):
        with pytest.raises(pkg.NdtError) as ei:
            pkg.alignVGICP(ndt, s["guess"])
        assert ei.value.code == code
        r, info = pkg.Result(), pkg.VgicpInfo()
        g = np.ascontiguousarray(guess_bits.T.ravel())
        assert L.ndt_align_vgicp(ndt._h, g.ctypes.data_as(C.POINTER(C.c_float)), C.byref(r), C.byref(info)) == code
        assert r.converged == 0 and np.array_equal(np.array(r.final_transformation[:], np.float32), g)
        assert info.n_voxels == 0 and info.n_pairs == 0

    # without a target, without a source
    assert code_of(pkg, pkg.evalDerivativesVGICP, C0, np.zeros(6)) == NO_TARGET
    assert code_of(pkg, pkg.vgicpInfo, C0) == NO_TARGET and code_of(pkg, pkg.vgicpVoxels, C0) == NO_TARGET
    align_leaves_the_guess(C0, NO_TARGET)
    C0.setInputTarget(s["target"])
    assert code_of(pkg, pkg.evalDerivativesVGICP, C0, np.zeros(6)) == NO_SOURCE
    align_leaves_the_guess(C0, NO_SOURCE)
    assert pkg.vgicpInfo(C0)["n_voxels"] > 0                                  # the table needs no source
    # a source none of whose points has a covariance
    C0.setInputSource(s["ideal"][:3])
    assert code_of(pkg, pkg.evalDerivativesVGICP, C0, np.zeros(6)) == NO_SOURCE
    align_leaves_the_guess(C0, NO_SOURCE)
    assert pkg.vgicpInfo(C0)["n_source_without_covariance"] == 3
    C0.setInputSource(s["ideal"])
    assert pkg.evalDerivativesVGICP(C0, POSE_GENERAL)[0]["n_pairs"] > 0
    # argument errors on a live handle
    words = np.zeros(32)
    dp = C.POINTER(C.c_double)
    pose = np.zeros(6)
    assert L.ndt_eval_derivatives_vgicp(C0._h, pose.ctypes.data_as(dp), 0, 1, words.ctypes.data_as(dp)) == INVALID_ARG
    assert L.ndt_eval_derivatives_vgicp(C0._h, None, 1, 1, words.ctypes.data_as(dp)) == INVALID_ARG
    bad = np.array([0, 0, 0, np.inf, 0, 0.0])
    assert L.ndt_eval_derivatives_vgicp(C0._h, bad.ctypes.data_as(dp), 1, 1, words.ctypes.data_as(dp)) == INVALID_ARG
    assert L.ndt_vgicp_export_voxels(C0._h, None, None, None, 1) == INVALID_ARG      # cap < n_leaves
    assert not words.any()
    # the search methods that are not a voxel lookup
    for method in (pkg.KDTREE, pkg.DIRECT26):
        C0.setNeighborhoodSearchMethod(method)
        assert code_of(pkg, pkg.evalDerivativesVGICP, C0, np.zeros(6)) == UNSUPPORTED
        align_leaves_the_guess(C0, UNSUPPORTED)
    C0.setNeighborhoodSearchMethod(pkg.DIRECT1)
    assert pkg.evalDerivativesVGICP(C0, POSE_GENERAL)[0]["n_pairs"] > 0
    # a target that keeps no points
    t = np.ascontiguousarray(s["target"].T)
    d = [hipmem.upload(t[a]) for a in range(3)]
    C0.setInputTargetDevice(d[0], d[1], d[2], len(s["target"]))
    assert code_of(pkg, pkg.evalDerivativesVGICP, C0, np.zeros(6)) == UNSUPPORTED
    assert code_of(pkg, pkg.vgicpInfo, C0) == UNSUPPORTED and code_of(pkg, pkg.vgicpVoxels, C0) == UNSUPPORTED
    align_leaves_the_guess(C0, UNSUPPORTED)
    # a multi-grid union
    U = engine(pkg)
    U.setInputSource(s["ideal"])
    U.addTarget(s["target"][:5000], 1)
    U.addTarget(s["target"][5000:], 2)
    U.createVoxelKdtree()
    assert code_of(pkg, pkg.evalDerivativesVGICP, U, np.zeros(6)) == UNSUPPORTED
    align_leaves_the_guess(U, UNSUPPORTED)


# ---- 5. the C++ adapter -------------------------------------------------------------------------------------------------------
def test_cpp_adapter(pkg, rig, tmp_path):
    """tests/cpp/test_vgicp.cpp against the API mocks, built with the g++ line tests/test_gpu_gicp.py uses; it reads the scene
    from a file this test writes and prints the final transformation, which must be the Python call's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "tests", "cpp")
    exe = str(tmp_path / "test_vgicp")
    lib = os.path.join(root, "slam-sam_amd", "libndt_hip.so")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-Wall", "-I" + os.path.join(d, "mock"),
                           "-I" + os.path.join(root, "include", "compat"), "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(d, "test_vgicp.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    blob = str(tmp_path / "scene.bin")
    with open(blob, "wb") as f:
        np.array([len(rig["target"]), len(rig["ideal"])], np.int64).tofile(f)
        rig["guess"].T.ravel().astype(np.float64).tofile(f)                             # column-major
        rig["target"].astype(np.float32).tofile(f)
        rig["ideal"].astype(np.float32).tofile(f)
    p = subprocess.run([exe, blob], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "vgicp: PASS" in p.stdout
    A = rig["A"]
    defaults(pkg, A)
    A.setInputSource(rig["ideal"])
    A.setNeighborhoodSearchMethod(pkg.DIRECT1)
    try:
        T, r = pkg.alignVGICP(A, rig["guess"])
    finally:
        A.setNeighborhoodSearchMethod(pkg.DIRECT7)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("final ")][0]
    col = np.array([float.fromhex(w) for w in line.split()[1:]]).reshape(4, 4).T
    assert np.array_equal(col, T)                                                       # the same engine, the same bits
