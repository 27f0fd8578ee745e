"""The sharded evaluation at 3 .. 7 ranks, ragged shards and every reducer that runs on one device.

Several processes share the one MI355X of the test box; each owns a handle, the (replicated) voxel table and a contiguous
shard of the source, and the 32-word evaluation is summed across them through NDT_REDUCE_HOOK, NDT_REDUCE_SHM and
NDT_REDUCE_P2P (RCCL refuses several ranks on one device).  tests/test_gpu_multiproc.py runs 2 ranks on even halves; here
the layouts are 3 / 4 / 7 even ranks, a ragged one with an empty, a 1-, 63-, 64- and 65-point shard beside a large one,
one with all points on the middle rank, and the C3 scan split 150 000 / 50 000 / 0.

The instrument is the hook reducer: the engine hands the hook a rank's LOCAL 32 words and takes the global sum back, so
the hook (over pkg.ranks.Board.allgather, two gathers of 16 doubles, summed in rank order from 0.0) is a transport under
test and the probe that records every rank's pre-reduction row.  With the evaluation log on (ndt_debug_eval_log) every
rank of every transport also records pose, f32 transform and the raw words after the cross-rank sum, before finish_eval.
After the ranks have exited the parent asserts:

  A  the reduce IS the rank-ordered f64 sum: the hook's sums and the logged words of the hook, shm and p2p runs equal the
     numpy sum of the recorded local rows, as uint64 bit patterns, on every rank; poses and transforms are bit-identical
     across ranks and transports;
  B  every recorded local row against the oracle's f64 statement of the same evaluation on that shard alone (pair_mode 2):
     counts exact, score / NVTL sum / Hessian / gradient by the compare() rule of tests/test_gpu_launch_shapes.py at its
     1e-9, the gradient relative to the largest oracle gradient norm of the global evaluations compared together.  Shards
     of fewer than TINY points (the 1 / 63 / 64 / 65 of `ragged6`) have scores near or at 0 -- a handful of points, some
     without any neighbour --, so a relative error of their own score says nothing: their score and Hessian are scaled by
     the smallest |score| / Hessian norm of the global evaluations compared together (the strictest of them).  An empty
     shard's rows are exactly 32 zero bit patterns.  The Hessian of the C3 shards' local rows is held to C3_LOCAL_H_TOL
     = 1.66e-8, twice the oracle's own f32-against-f64 spread there (measured 8.3e-9; see the constant), where 1e-9 gave
     1.1e-9;
  C  the summed row against the oracle on the whole source (batches: first, last and both sides of each 64-pose round);
  D  what is applied once after the sum: transform_probability over the global size, NVTL = global sum / global count,
     n_pairs, finish_eval's regularisation (numpy restatement in f32, bit for bit: score of every history entry, score and
     Hessian of the result) weighted by the GLOBAL n_pairs, the ridge of the SVN preset exactly once;
  E  sharded == unsharded where promised (bit-identical across ranks and transports; against a single-process align within
     the bounds of test_two_processes_one_gpu_shm_reduction);
  F  the per-shard calls (scorePoints, filterSource, fitness) are the unsharded call restricted to the shard;
  G  P2P housekeeping without timing claims (late / host-finish counts are printed, not asserted: seven processes share
     one device and a rank that is 20 ms late is finished on the host by design -- A .. E prove that path changed no bit).

A hook call whose summed word 31 is raised (a pre-launched kernel that gave up waiting for its pose on a crowded device:
the evaluation is repeated, ndt_evaluate.hip) has no log entry and is left out of the pairing.
"""
import math
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
TINY = 1000
TRANSPORTS = ("hook", "shm", "p2p")
REG_SCALE = 0.01
SVN_K, SVN_ITERS, SVN_SEED = 20, 3, 5
# The Hessian of a LOCAL row of the C3 shards (0.5 m voxels), the one place where the project's 1e-9 does not hold: a shard of
# 150 000 points came out at 1.1e-9 of its own Hessian norm at one of the 130 perturbed poses (score 3.5e-10, gradient
# 8.7e-11; the global rows, and every row of the C2 layouts, are within 1e-9).  The differences between kernel and oracle
# are roundings of single terms, which average out with the number of pairs -- a pure difference of f64 summation order
# would sit near 1e-14 --, so a shard's relative error is larger than that of the whole scan the 1e-9 was set on, and the
# Hessian, whose terms carry the f32 angle tables and lever arms of tens of metres, is the first word to cross it.  The
# yardstick is the ORACLE's own f32-against-f64 spread on these inputs (pair_mode 0 against pair_mode 2: the reference's
# f32 products against the same formulas in f64), measured on the CPU at the ground-truth pose, the 5 and every fourth of
# the 130 perturbed poses of this module: relative Hessian difference, median 1.0e-8 on the 150 000-point shard (range
# 2.0e-10 .. 8.7e-8) and 8.3e-9 on the 50 000-point one (7.0e-10 .. 1.4e-7); the score's spread is 0 and the gradient's
# median 2.3e-10 of the gradient scale, so both keep 1e-9.  Bound: twice the smaller median.
C3_LOCAL_H_TOL = 2 * 8.3e-9
ROUND = 64   # poses per P2P batch round (XCHG_BATCH_MAX, csrc/ndt_device.h)

# id -> (workload, world, shard sizes: None = ndt_shard_range, -1 = the rest of the source)
LAYOUTS = {
    "even3": ("c2", 3, None),
    "even4": ("c2", 4, None),
    "even7": ("c2", 7, None),
    "ragged6": ("c2", 6, [0, 1, 63, 64, 65, -1]),
    "lonely3": ("c2", 3, [0, -1, 0]),
    "c3big3": ("c3", 3, [150000, 50000, 0]),
}


# ---- helpers without a GPU (tests/test_sharded_cpu.py checks them) --------------------------------------------------

def layout_shards(name, n, shard_range):
    """Shard sizes of layout `name` for a source of n points, in rank order; shard_range: pkg.shard_range."""
    _, world, sizes = LAYOUTS[name]
    if sizes is None:
        out, at = [], 0
        for r in range(world):
            b, c = shard_range(n, r, world)
            assert b == at, (name, r, b, at)
            out.append(int(c))
            at += c
        return out
    fixed = sum(s for s in sizes if s >= 0)
    assert sizes.count(-1) <= 1 and fixed <= n, (name, n)
    return [int(s) if s >= 0 else int(n - fixed) for s in sizes]


def shard_bounds(sizes):
    """[(begin, count)] of contiguous shards."""
    out, at = [], 0
    for s in sizes:
        out.append((at, int(s)))
        at += int(s)
    return out


def rank_ordered_sum(rows):
    """s = 0.0; for r: s += rows[r] -- the order of allreduce_host, allreduce_host_batch, p2p_finish_on_host and
    xchg_allsum.  rows: [world, n] float64."""
    rows = np.asarray(rows, dtype=np.float64)
    s = np.zeros(rows.shape[1], dtype=np.float64)
    for r in range(rows.shape[0]):
        s = s + rows[r]
    return s


def bits(w):
    return np.ascontiguousarray(w, dtype=np.float64).view(np.uint64)


def unpack_words(w):
    """32 words -> (score, g[6], H[6, 6]) as ndt_unpack_eval does."""
    w = np.asarray(w, dtype=np.float64)
    H = np.zeros((6, 6))
    k = 7
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = w[k]
            k += 1
    return float(w[0]), w[1:7].copy(), H


def finish_eval_np(words, pose6, need_h, add_ridge=False, reg_pose=None, scale=0.0):
    """finish_eval (csrc/ndt_newton.cpp) restated: the ridge, then the longitudinal regularisation in f32 arithmetic,
    operation by operation as written there (the library is built with -ffp-contract=off), weighted by the n_pairs
    word.  reg_pose: 4 x 4.  Returns (score, g, H)."""
    f = np.float32
    score, g, H = unpack_words(words)
    if need_h and add_ridge:
        for i in range(6):
            H[i, i] += 1e-6
    if reg_pose is not None:
        rp = np.asarray(reg_pose, dtype=np.float32)
        k = f(scale)
        dx = f(rp[0, 3] - f(pose6[0]))
        dy = f(rp[1, 3] - f(pose6[1]))
        sy, cy = f(math.sin(pose6[5])), f(math.cos(pose6[5]))
        lon = f(f(dy * sy) + f(dx * cy))
        wgt = f(words[30])
        two = f(2.0)
        kw = f(k * wgt)
        nkw = f(f(-k) * wgt)
        score += float(f(f(nkw * lon) * lon))
        g[0] += float(f(f(f(kw * two) * cy) * lon))
        g[1] += float(f(f(f(kw * two) * sy) * lon))
        if need_h:
            H[0, 0] += float(f(f(f(nkw * two) * cy) * cy))
            xy = float(f(f(f(nkw * two) * cy) * sy))
            H[0, 1] += xy
            H[1, 0] += xy
            H[1, 1] += float(f(f(f(nkw * two) * sy) * sy))
    return score, g, H


def sampled(K):
    """indices of a batch of K poses that are compared with the oracle on the whole source"""
    idx = {0, K - 1}
    for b in range(ROUND, K, ROUND):
        idx.update((b - 1, b))
    return sorted(i for i in idx if 0 <= i < K)


# ---- the rank ----------------------------------------------------------------------------------------------------------

def _log_arrays(log):
    n = len(log)
    return dict(pose6=np.array([e["pose6"] for e in log]).reshape(n, 6), words=np.array([e["words"] for e in log]).reshape(n, 32),
                T32=np.array([e["T32"] for e in log], dtype=np.float32).reshape(n, 16),
                need_h=np.array([e["need_h"] for e in log], dtype=bool), score_only=np.array([e["score_only"] for e in log], dtype=bool),
                K=np.array([e["K"] for e in log], dtype=np.int64), k=np.array([e["k"] for e in log], dtype=np.int64),
                mode=np.array([e["desc"]["mode"] for e in log], dtype=np.int64),
                threads=np.array([e["desc"]["threads"] for e in log], dtype=np.int64))


def _evals(es):
    return dict(score=np.array([e["score"] for e in es]), g=np.stack([e["gradient"] for e in es]),
                H=np.stack([e["hessian"] for e in es]))


def _worker(rank, world, name, out_dir, mode, cfg_path):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import __graft_entry__ as ge
    pkg = ge.load_package()
    z = np.load(cfg_path)
    target, source, guess, gt = z["target"], z["source"], z["guess"], z["gt"]
    begin, count = shard_bounds(z["sizes"])[rank]
    shard = source[begin:begin + count]
    min_score = float(z["min_score"])
    board = pkg.ranks.Board("/dev/shm" + name + "_board", rank, world, timeout=120)
    # (several engines on ONE device: pre-launched kernels stay on each engine's own stream, include/ndt_hip.h)
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=float(z["resolution"]), step_size=0.1, trans_epsilon=1e-4,
                                           max_iterations=35, prelaunch=pkg.PRELAUNCH_ONE_STREAM)
    ndt.setInputTarget(target)
    ndt.setInputSource(shard)
    ndt.setGlobalSourceSize(len(source))
    calls = []

    def hook(_ctx, words_p, n):
        try:
            w = np.ctypeslib.as_array(words_p, shape=(n,))
            loc = w.copy()
            halves = []
            for lo in range(0, n, 16):   # (the board's payload limit is 252 bytes)
                got = board.allgather(loc[lo:lo + 16].tobytes())
                halves.append(np.stack([np.frombuffer(b, dtype=np.float64) for b in got]))
            s = rank_ordered_sum(np.concatenate(halves, axis=1))
            w[:] = s
            calls.append((loc, s))
            return 0
        except Exception:
            import traceback
            traceback.print_exc()
            return 1

    if mode == "hook":
        ndt.commInitHook(hook, rank, world)
    elif mode == "p2p":
        ndt.commInitP2p(b"".join(board.allgather(ndt.commP2pHandle())), rank, world)
    else:
        ndt.commInitShm(name, rank, world)
    assert ndt.commRankCount() == world
    selftest = again = stats = None
    if mode == "p2p":
        selftest = ndt.commP2pSelftest(2000)
        board.barrier()
        ndt.commP2pStats(reset=True)
    ndt.debugEvalLog(4096)
    marks = [0]

    def mark():
        marks.append(len(ndt.debugEvalLogRead()))

    out = {}
    # 1. plain align
    T1 = ndt.align(guess)
    r1 = ndt.getResult()
    mark()
    # 2. the same align under the longitudinal regularisation (weighted by the GLOBAL n_pairs, once, after the sum)
    ndt.setRegularizationPose(gt)
    ndt.setRegularizationScaleFactor(REG_SCALE)
    T2 = ndt.align(guess)
    r2 = ndt.getResult()
    hT, htp, hnv = ndt.getIterationHistory()
    ndt.unsetRegularizationPose()
    ndt.setRegularizationScaleFactor(0.0)
    mark()
    # 3 .. 6. batches: one pose, 5 with the Hessian, 70 without (two P2P rounds), 130 with (three: the parity wraps)
    rng = np.random.default_rng(3)
    poses5 = r1["pose"] + rng.normal(0, 0.01, (5, 6))
    poses70 = r1["pose"] + rng.normal(0, 0.01, (70, 6))
    poses130 = r1["pose"] + rng.normal(0, 0.01, (130, 6))
    out["e1"] = _evals(ndt.evalDerivatives(r1["pose"]))
    mark()
    out["b5"] = _evals(ndt.evalDerivatives(poses5))
    mark()
    out["b70"] = _evals(ndt.evalDerivatives(poses70, compute_hessian=False))
    mark()
    out["b130"] = _evals(ndt.evalDerivatives(poses130))
    mark()
    # 7. score only: single pose (inside the kernel under P2P) and a batch
    S = pkg.synth
    Ts5 = [T1 @ S.pose_matrix(*d) for d in rng.normal(0, [0.02, 0.02, 0.01, 0.002, 0.002, 0.005], (5, 6))]
    sc = ndt.scoreTransform(T1)
    scs = ndt.scoreTransforms(Ts5)
    mark()
    # 8. a second plain align: the round tags keep counting behind the batches
    T3 = ndt.align(guess)
    r3 = ndt.getResult()
    mark()
    # 9. SVN: Stage 1 goes through allreduce_host_batch; then two evaluations under the same switches (the ridge)
    ndt.setParams(hessian_mode=pkg.HESSIAN_GAUSS_NEWTON, add_ridge=1)
    sp = pkg.SvnParams()
    pkg.lib().ndt_svn_default_params(C.byref(sp))
    sp.particle_count, sp.max_iterations = SVN_K, SVN_ITERS
    particles = pkg.svn_sample_particles(T1, SVN_K, SVN_SEED)
    part = np.ascontiguousarray(particles.transpose(0, 2, 1)).ravel().copy()
    prior = np.ascontiguousarray(np.asarray(T1, dtype=np.float64).T).ravel()
    sr = pkg.SvnResult()
    rc = pkg.lib().ndt_svn_align(ndt._h, C.byref(sp), prior.ctypes.data_as(C.POINTER(C.c_double)),
                                 part.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sr))
    assert rc == 0, (rc, pkg.lib().ndt_last_error(ndt._h))
    mark()
    out["ridge"] = _evals(ndt.evalDerivatives(poses5[:2]))
    ndt.setParams(hessian_mode=pkg.HESSIAN_FULL, add_ridge=0)
    mark()
    log = ndt.debugEvalLogRead()
    ndt.debugEvalLog(0)
    # 10. the unreduced per-shard calls
    pp = ndt.scorePoints(T1)
    fxyz, fidx = ndt.filterSource(T1, min_score)
    fit = ndt.fitness(T1, max_range=1.0, per_point=True)
    # 11. multi-rank batches of aligns are refused, and the guesses come back
    g2 = np.ascontiguousarray(np.stack([np.asarray(guess, dtype=np.float32).T.ravel(),
                                        np.asarray(gt, dtype=np.float32).T.ravel()]))
    res2 = (pkg.Result * 2)()
    rc_many = pkg.lib().ndt_align_batch(ndt._h, g2.ctypes.data_as(C.POINTER(C.c_float)), 2, res2)
    many_T = np.array([res2[k].final_transformation[:] for k in range(2)], dtype=np.float32)
    try:
        ndt.alignMany([guess, gt])
        many_code = 0
    except pkg.NdtError as e:
        many_code = e.code
    if mode == "p2p":
        stats = ndt.commP2pStats()
        board.barrier()
        again = ndt.commP2pSelftest(501)   # (odd: the last round sits in generation 1, where the next evaluation writes)
        board.barrier()
    save = dict(marks=np.array(marks), T1=T1, T2=T2, T3=T3, many_rc=rc_many, many_code=many_code, many_T=many_T, many_g=g2,
                poses5=poses5, poses70=poses70, poses130=poses130, Ts5=np.stack(Ts5),
                svn_pose=np.array(sr.final_pose[:]), svn_cov=np.array(sr.final_covariance[:]), svn_part=part,
                svn_iters=sr.iterations, hist_T=hT, hist_tp=htp, hist_nv=hnv,
                pp_score=pp["score"], pp_nvs=pp["nearest_voxel_score"], pp_nn=pp["n_neighbors"], pp_bv=pp["best_voxel"],
                f_xyz=fxyz, f_idx=fidx, fit_sq=fit["sq_dists"], fit_sum=fit["sum_sq_dist"], fit_in=fit["n_inliers"],
                fit_np=fit["n_points"], fit_score=fit["fitness_score"],
                sc=np.array([[s["score"], s["transform_probability"], s["nvtl"], s["n_pairs"], s["n_points_with_neighbors"]]
                             for s in [sc] + scs]),
                counters=np.array(ndt.prelaunchCounters()), finishes=ndt.p2pHostFinishes(), retries=ndt.lostRowRetries())
    for tag, r in (("r1", r1), ("r2", r2), ("r3", r3)):
        for k in ("pose", "hessian", "score", "transform_probability", "nvtl", "n_pairs", "n_points_with_neighbors", "iterations",
                  "n_evaluations", "n_evaluations_reused", "converged"):
            save["%s_%s" % (tag, k)] = r[k]
    for tag, d in out.items():
        for k, v in d.items():
            save["%s_%s" % (tag, k)] = v
    for k, v in _log_arrays(log).items():
        save["log_" + k] = v
    if mode == "hook":
        save["hook_loc"] = np.array([c[0] for c in calls]).reshape(len(calls), 32)
        save["hook_sum"] = np.array([c[1] for c in calls]).reshape(len(calls), 32)
    if mode == "p2p":
        save.update(st_exchanges=stats["exchanges"], st_late=stats["late"], st_max_us=stats["max_us"],
                    sel=np.array([selftest["rounds"], selftest["torn"], selftest["missed"]]),
                    sel2=np.array([again["rounds"], again["torn"], again["missed"]]))
    np.savez(os.path.join(out_dir, "%s_rank%d.npz" % (mode, rank)), **save)
    board.barrier()   # nobody unmaps a peer's area (or leaves the board) while a peer may still write into it
    ndt.commDestroy()
    ndt.close()
    board.close()


# ---- the parent ----------------------------------------------------------------------------------------------------------

class Ref:
    """Per workload: the oracle's grid, a single-process handle on the whole source and its align (made before any rank
    starts; the per-point reference calls are made after the ranks have exited)."""

    def __init__(self, pkg, O, S, name):
        self.name = name
        self.cfg = S.config_c2() if name == "c2" else S.config_c3()
        self.res = 1.0 if name == "c2" else 0.5
        kw = dict(resolution=self.res, step_size=0.1, trans_epsilon=1e-4)
        self.prm = {gn: O.default_params(num_threads=16, pair_mode=2, max_iterations=35, hessian_mode=gn, **kw) for gn in (0, 1)}
        self.grid = O.Grid(self.cfg["target"], self.prm[0])
        self.ndt = pkg.NormalDistributionsTransform(device_id=0, max_iterations=35, **kw)
        self.ndt.setInputTarget(self.cfg["target"])
        self.ndt.setInputSource(self.cfg["source"])
        self.T = self.ndt.align(self.cfg["guess"])
        self.r = self.ndt.getResult()
        self.min_score = float(np.median(self.ndt.scorePoints(self.T, fields=["nearest_voxel_score"])["nearest_voxel_score"]))
        self.memo = {}

    def oracle(self, begin, count, pose6, T32, need_h, gn):
        k = (begin, count, pose6.tobytes(), T32.tobytes(), bool(need_h), int(gn))
        if k not in self.memo:
            T = np.asarray(T32, dtype=np.float64).reshape(4, 4).T
            self.memo[k] = self.grid.derivatives(self.cfg["source"][begin:begin + count], pose6, T=T, compute_hessian=bool(need_h),
                                                 params=self.prm[int(gn)])
        return self.memo[k]


@pytest.fixture(scope="module")
def refs(pkg, O, S):
    n, info = pkg.backend_info()
    assert n > 0, "GPU test on a box without a HIP device: " + info
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Ref(pkg, O, S, name)
        return cache[name]

    yield get
    for r in cache.values():
        r.ndt.close()


def _run_ranks(world, mode, out_dir, cfg_path, tag):
    """Starts the ranks, joins them within 600 s; one rank failing or late ends the others and the test."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    name = "/ndt_shard_%s_%s_%d" % (tag, mode, os.getpid())
    old = os.environ.get("NDT_COMM_TIMEOUT_S")
    os.environ["NDT_COMM_TIMEOUT_S"] = "30"    # inherited by the ranks: a missing peer ends the run quickly
    try:
        procs = [ctx.Process(target=_worker, args=(r, world, name, out_dir, mode, cfg_path)) for r in range(world)]
        for p in procs:
            p.start()
    finally:
        if old is None:
            os.environ.pop("NDT_COMM_TIMEOUT_S", None)
        else:
            os.environ["NDT_COMM_TIMEOUT_S"] = old
    t0 = time.monotonic()
    bad = None
    while bad is None and any(p.exitcode is None for p in procs):
        for r, p in enumerate(procs):
            p.join(0.05)
            if p.exitcode not in (None, 0):
                bad = "rank %d exited with %s" % (r, p.exitcode)
                break
        if bad is None and time.monotonic() - t0 > 600:
            bad = "ranks still running after 600 s"
    if bad is None:
        bad = next(("rank %d exited with %s" % (r, p.exitcode) for r, p in enumerate(procs) if p.exitcode != 0), None)
    if bad is not None:
        for p in procs:
            if p.exitcode is None:
                p.terminate()
        for p in procs:
            p.join(15)
            if p.exitcode is None:
                p.kill()
                p.join(5)
        for path in ("/dev/shm" + name + "_board", "/dev/shm" + name):
            try:
                os.unlink(path)
            except OSError:
                pass
        pytest.fail("%s %s: %s" % (tag, mode, bad), pytrace=False)
    return [dict(np.load(os.path.join(out_dir, "%s_rank%d.npz" % (mode, r)))) for r in range(world)]


def _got(w):
    s, g, H = unpack_words(w)
    return dict(score=s, gradient=g, hessian=H, nvtl_sum=float(w[28]), n_with_neighbors=int(w[29]), n_pairs=int(w[30]))


def _compare(got, d, gscale, need_h, score_only, what, worst, sscale=None, hscale=None, htol=None):
    """compare() of tests/test_gpu_launch_shapes.py; score-only rows carry no gradient; sscale / hscale: the global
    evaluation's scales for a tiny shard (module docstring, B); htol: the Hessian's bound where it is not TOL."""
    from test_gpu_launch_shapes import compare
    if not score_only and sscale is None and htol is None:
        compare(got, d, gscale, need_h, what, tol=TOL, worst=worst)
        return
    assert got["n_pairs"] == d["n_pairs"], (what, got["n_pairs"], d["n_pairs"])
    assert got["n_with_neighbors"] == d["n_with_neighbors"], (what, got["n_with_neighbors"], d["n_with_neighbors"])
    assert abs(got["nvtl_sum"] - d["nvtl_sum"]) <= TOL * abs(d["nvtl_sum"]) + 1e-9, (what, got["nvtl_sum"], d["nvtl_sum"])
    es = abs(got["score"] - d["score"]) / (sscale if sscale is not None else abs(d["score"]))
    eg = 0.0 if score_only else np.linalg.norm(got["gradient"] - d["gradient"]) / gscale
    eh = 0.0
    if need_h and not score_only:
        eh = np.linalg.norm(got["hessian"] - d["hessian"]) / (hscale if hscale is not None else np.linalg.norm(d["hessian"]))
    for k, v in (("score", es), ("g", eg), ("H", eh)):
        worst[k] = max(worst.get(k, 0.0), v)
    assert es < TOL and eg < TOL and eh < (TOL if htol is None else htol), (what, es, eg, eh)


STEPS = ("align", "align_reg", "batch1", "batch5", "batch70", "batch130", "score", "align2", "svn", "ridge")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_sharded_layout(pkg, O, S, refs, tmp_path, layout):
    wl, world, _ = LAYOUTS[layout]
    ref = refs(wl)
    cfg = ref.cfg
    n = len(cfg["source"])
    sizes = layout_shards(layout, n, pkg.shard_range)
    bounds = shard_bounds(sizes)
    assert sum(sizes) == n and len(sizes) == world
    cfg_path = os.path.join(str(tmp_path), "cfg.npz")
    np.savez(cfg_path, target=cfg["target"], source=cfg["source"], guess=cfg["guess"], gt=cfg["gt"], sizes=np.array(sizes),
             resolution=ref.res, min_score=ref.min_score)
    runs = {}
    for mode in TRANSPORTS:
        d = os.path.join(str(tmp_path), mode)
        os.makedirs(d)
        runs[mode] = _run_ranks(world, mode, d, cfg_path, layout)
    hook = runs["hook"]
    base = hook[0]
    N = len(base["log_words"])
    marks = [int(m) for m in base["marks"]]
    assert len(marks) == len(STEPS) + 1 and marks[-1] == N
    step_of = np.zeros(N, dtype=np.int64)
    for s in range(len(STEPS)):
        step_of[marks[s]:marks[s + 1]] = s
    K_of = {"batch1": 1, "batch5": 5, "batch70": 70, "batch130": 130}
    for s, nm in enumerate(STEPS):
        if nm in K_of:
            assert marks[s + 1] - marks[s] == K_of[nm] and np.all(base["log_K"][marks[s]:marks[s + 1]] == K_of[nm]), nm
    assert marks[9] - marks[8] == SVN_K * int(base["svn_iters"]) and int(base["svn_iters"]) >= 1
    assert marks[7] - marks[6] == 1 + 5 and np.all(base["log_score_only"][marks[6]:marks[7]])
    assert np.all(base["log_mode"][marks[8]:marks[10]] == 2)     # Gauss-Newton under the SVN preset

    # ---- A: the reduce is the rank-ordered f64 sum, bit for bit; poses agree everywhere
    loc = []
    for r in range(world):
        keep = (hook[r]["hook_sum"][:, 31] == 0.0) & ~np.isnan(hook[r]["hook_sum"]).any(axis=1)   # (repeated evaluations: docstring)
        assert int(keep.sum()) == N, (layout, r, int(keep.sum()), N, len(keep))
        loc.append(hook[r]["hook_loc"][keep])
        hook[r]["hook_sum_kept"] = hook[r]["hook_sum"][keep]
    loc = np.stack(loc)                                      # [world, N, 32]
    want = np.stack([rank_ordered_sum(loc[:, i, :]) for i in range(N)])
    assert not np.isnan(want).any()
    for r in range(world):
        assert np.array_equal(bits(hook[r]["hook_sum_kept"]), bits(want)), (layout, "hook sum", r)
    for mode in TRANSPORTS:
        for r in range(world):
            z = runs[mode][r]
            assert len(z["log_words"]) == N, (layout, mode, r, len(z["log_words"]), N)
            bad = np.nonzero((bits(z["log_words"]) != bits(want)).any(axis=1))[0]
            assert len(bad) == 0, (layout, mode, r, "logged words != rank-ordered sum at evaluations", bad[:8],
                                   [STEPS[step_of[i]] for i in bad[:8]])
            assert np.array_equal(bits(z["log_pose6"]), bits(base["log_pose6"])), (layout, mode, r, "pose6")
            assert np.array_equal(z["log_T32"].view(np.uint32), base["log_T32"].view(np.uint32)), (layout, mode, r, "T32")
            for k in ("log_need_h", "log_score_only", "log_K", "log_k", "log_mode", "marks"):
                assert np.array_equal(z[k], base[k]), (layout, mode, r, k)
    # the launch shapes that met in one exchange
    shapes = sorted({int(hook[r]["log_threads"][0]) for r in range(world)})

    # ---- C: the global row against the oracle on the whole source
    cset = []
    for i in range(N):
        K, k = int(base["log_K"][i]), int(base["log_k"][i])
        if K == 1 or k in sampled(K):
            cset.append(i)

    def orc(i, b, c):
        return ref.oracle(b, c, base["log_pose6"][i], base["log_T32"][i], base["log_need_h"][i], base["log_mode"][i] == 2)

    glob = {i: orc(i, 0, n) for i in cset}
    grad_set = [i for i in cset if not base["log_score_only"][i]]
    gscale = max(np.linalg.norm(glob[i]["gradient"]) for i in grad_set)
    sscale = min(abs(glob[i]["score"]) for i in cset)
    hscale = min(np.linalg.norm(glob[i]["hessian"]) for i in grad_set if base["log_need_h"][i])
    worst_g, worst_l = {}, {}
    for i in cset:
        _compare(_got(want[i]), glob[i], gscale, bool(base["log_need_h"][i]), bool(base["log_score_only"][i]),
                 (layout, "global", STEPS[step_of[i]], i), worst_g)

    # ---- B: every rank's local row against the oracle on that shard alone
    n_local = 0
    for r, (b, c) in enumerate(bounds):
        if c == 0:
            assert not bits(loc[r]).any(), (layout, r, "an empty shard's rows are 32 zeros")
            continue
        tiny = c < TINY
        for i in range(N):
            _compare(_got(loc[r, i]), orc(i, b, c), gscale, bool(base["log_need_h"][i]), bool(base["log_score_only"][i]),
                     (layout, "local", r, c, STEPS[step_of[i]], i), worst_l,
                     sscale=sscale if tiny else None, hscale=hscale if tiny else None,
                     htol=C3_LOCAL_H_TOL if wl == "c3" else None)
            n_local += 1

    # ---- D: what is applied once, after the sum
    def last_of(step):
        return marks[STEPS.index(step) + 1] - 1

    for mode in TRANSPORTS:
        for r in range(world):
            z = runs[mode][r]
            for tag, step in (("r1", "align"), ("r2", "align_reg"), ("r3", "align2")):
                w = want[last_of(step)]
                assert float(z[tag + "_transform_probability"]) == float(z[tag + "_score"]) / n, (layout, mode, r, tag)
                assert float(z[tag + "_nvtl"]) == w[28] / w[29], (layout, mode, r, tag)
                assert int(z[tag + "_n_pairs"]) == int(w[30]) and int(z[tag + "_n_points_with_neighbors"]) == int(w[29])
                assert int(z[tag + "_n_evaluations"]) == marks[STEPS.index(step) + 1] - marks[STEPS.index(step)]
            # plain aligns: finish_eval adds nothing
            for tag, step in (("r1", "align"), ("r3", "align2")):
                s, g, H = unpack_words(want[last_of(step)])
                assert float(z[tag + "_score"]) == s and np.array_equal(bits(z[tag + "_hessian"]), bits(H)), (layout, mode, r, tag)
            # the regularised align: finish_eval of the raw summed words (global n_pairs), bit for bit
            i = last_of("align_reg")
            s, g, H = finish_eval_np(want[i], base["log_pose6"][i], True, reg_pose=cfg["gt"], scale=REG_SCALE)
            assert bits(np.array([float(z["r2_score"])]))[0] == bits(np.array([s]))[0], (layout, mode, r, float(z["r2_score"]), s)
            assert np.array_equal(bits(z["r2_hessian"]), bits(H)), (layout, mode, r, "regularised Hessian")
            assert s != want[i][0] and not np.array_equal(H, unpack_words(want[i])[2])   # (the term is not nothing)
            lo, hi = marks[1], marks[2]
            assert len(z["hist_tp"]) >= 2
            for T, tp, nv in zip(z["hist_T"], z["hist_tp"], z["hist_nv"]):
                T16 = np.ascontiguousarray(np.asarray(T, dtype=np.float32).T).ravel()
                hit = [j for j in range(lo, hi) if np.array_equal(base["log_T32"][j], T16)]
                assert hit, (layout, mode, r, "history transform not among the logged evaluations")
                j = hit[-1]
                s = finish_eval_np(want[j], base["log_pose6"][j], True, reg_pose=cfg["gt"], scale=REG_SCALE)[0]
                assert tp == s / n and nv == want[j][28] / want[j][29], (layout, mode, r, j)
            # unregularised batches: the finished values are the raw sums
            for tag, step in (("e1", "batch1"), ("b5", "batch5"), ("b70", "batch70"), ("b130", "batch130")):
                a = marks[STEPS.index(step)]
                for k in range(len(z[tag + "_score"])):
                    s, g, H = unpack_words(want[a + k])
                    assert z[tag + "_score"][k] == s and np.array_equal(bits(z[tag + "_g"][k]), bits(g)), (layout, mode, r, tag, k)
                    assert np.array_equal(bits(z[tag + "_H"][k]), bits(H)), (layout, mode, r, tag, k)
            # the SVN preset: +1e-6 on the Hessian's diagonal, once
            a = marks[STEPS.index("ridge")]
            for k in range(2):
                s, g, H = finish_eval_np(want[a + k], base["log_pose6"][a + k], True, add_ridge=True)
                assert np.array_equal(bits(z["ridge_H"][k]), bits(H)) and z["ridge_score"][k] == s, (layout, mode, r, "ridge", k)
                assert np.array_equal(bits(np.diag(H)), bits(np.diag(unpack_words(want[a + k])[2]) + 1e-6))
            # score only
            a = marks[STEPS.index("score")]
            for k in range(6):
                w = want[a + k]
                assert np.array_equal(z["sc"][k], np.array([w[0], w[0] / n, w[28] / w[29], w[30], w[29]])), (layout, mode, r, "score", k)
            # ndt_align_batch under a reducer
            assert int(z["many_rc"]) == -9 and int(z["many_code"]) == -9, (layout, mode, r, int(z["many_rc"]), int(z["many_code"]))
            assert np.array_equal(z["many_T"], z["many_g"]), (layout, mode, r, "the guesses come back")

    # ---- E: sharded == unsharded where promised
    keys = ["T1", "T2", "T3", "svn_pose", "svn_cov", "svn_part", "svn_iters"] + \
           ["%s_%s" % (t, k) for t in ("r1", "r2", "r3") for k in ("hessian", "iterations", "n_evaluations", "pose", "score")]
    for mode in TRANSPORTS:
        for r in range(world):
            for k in keys:
                a, b = runs[mode][r][k], base[k]
                same = np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
                assert same, (layout, mode, r, k)
    assert np.array_equal(bits(base["T3"]), bits(base["T1"])) and np.array_equal(bits(base["r3_hessian"]), bits(base["r1_hessian"]))
    assert int(base["r3_iterations"]) == int(base["r1_iterations"]) and int(base["r3_n_evaluations"]) == int(base["r1_n_evaluations"])
    dt, dr = S.pose_error(base["T1"], ref.T)
    assert dt < 1e-5 and dr < 1e-6, (layout, dt, dr)
    assert abs(int(base["r1_n_pairs"]) - int(ref.r["n_pairs"])) <= max(2, 1e-4 * ref.r["n_pairs"])
    assert float(base["r1_transform_probability"]) == pytest.approx(ref.r["transform_probability"], rel=1e-6)

    # ---- F: the per-shard calls are the unsharded call restricted to the shard (any transport: they are not reduced)
    T1 = base["T1"]
    upp = ref.ndt.scorePoints(T1)
    uxyz, uidx = ref.ndt.filterSource(T1, ref.min_score)
    ufit = ref.ndt.fitness(T1, max_range=1.0, per_point=True)
    assert 0 < len(uidx) < n
    for mode in TRANSPORTS:
        zs = runs[mode]
        for r, (b, c) in enumerate(bounds):
            assert len(zs[r]["pp_score"]) == c and len(zs[r]["fit_sq"]) == c and int(zs[r]["fit_np"]) <= c
            if c == 0:
                assert int(zs[r]["fit_np"]) == 0 and int(zs[r]["fit_in"]) == 0 and len(zs[r]["f_idx"]) == 0
        for k, u in (("pp_score", "score"), ("pp_nvs", "nearest_voxel_score"), ("pp_nn", "n_neighbors"), ("pp_bv", "best_voxel")):
            cat = np.concatenate([zs[r][k] for r in range(world)])
            assert cat.dtype == upp[u].dtype and np.array_equal(cat.view(np.uint8), upp[u].view(np.uint8)), (layout, mode, u)
        sq = np.concatenate([zs[r]["fit_sq"] for r in range(world)])
        assert np.array_equal(sq.view(np.uint32), ufit["sq_dists"].view(np.uint32)), (layout, mode, "sq_dists")
        assert sum(int(zs[r]["fit_in"]) for r in range(world)) == ufit["n_inliers"]
        assert sum(int(zs[r]["fit_np"]) for r in range(world)) == ufit["n_points"]
        ssum = rank_ordered_sum(np.array([[float(zs[r]["fit_sum"])] for r in range(world)]))[0]
        assert abs(ssum - ufit["sum_sq_dist"]) <= 1e-12 * abs(ufit["sum_sq_dist"]), (layout, mode, ssum, ufit["sum_sq_dist"])
        idx = np.concatenate([zs[r]["f_idx"].astype(np.int64) + bounds[r][0] for r in range(world)])
        assert np.array_equal(idx, uidx.astype(np.int64)), (layout, mode, "filterSource indices")
        assert np.array_equal(np.concatenate([zs[r]["f_xyz"] for r in range(world)]), uxyz), (layout, mode, "filterSource points")

    # ---- G: P2P housekeeping, without timing claims
    late = finishes = 0
    for r in range(world):
        z = runs["p2p"][r]
        assert list(z["sel"]) == [2000, 0, 0] and list(z["sel2"]) == [501, 0, 0], (layout, r, z["sel"], z["sel2"])
        assert int(z["st_exchanges"]) > 0
        late += int(z["st_late"])
        finishes += int(z["finishes"])
    print("\n%s (%s, world %d, shards %s, block threads %s): %d evaluations per rank and transport" %
          (layout, wl, world, sizes, shapes, N))
    print("  global rows vs oracle: %d compared, worst score %.1e  g %.1e  H %.1e" %
          (len(cset), worst_g.get("score", 0), worst_g.get("g", 0), worst_g.get("H", 0)))
    print("  local rows vs oracle:  %d compared, worst score %.1e  g %.1e  H %.1e" %
          (n_local, worst_l.get("score", 0), worst_l.get("g", 0), worst_l.get("H", 0)))
    for mode in TRANSPORTS:
        zs = runs[mode]
        print("  %-4s every rank's %d logged rows == the rank-ordered sum bit for bit; pre-launch (used, quit, time-outs) %s, "
              "lost-row retries %s" % (mode, N, [tuple(int(v) for v in zs[r]["counters"]) for r in range(world)],
                                       [int(zs[r]["retries"]) for r in range(world)]))
    print("  p2p: late %d, host finishes %d" % (late, finishes))


# ---- in-process, one handle ------------------------------------------------------------------------------------------------

def _small(pkg, S):
    cfg = S.config_c1(max_points=20000)
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=30)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    return cfg, ndt


def _logged_run(ndt, cfg):
    ndt.debugEvalLog(512)
    T = ndt.align(cfg["guess"])
    r = ndt.getResult()
    n_align = len(ndt.debugEvalLogRead())
    rng = np.random.default_rng(1)
    b = ndt.evalDerivatives(r["pose"] + rng.normal(0, 0.01, (3, 6)))
    log = ndt.debugEvalLogRead()
    ndt.debugEvalLog(0)
    return T, r, b, log, n_align


def test_hook_world_one_identity(pkg, S, refs):
    """A one-rank hook that changes nothing: the align is the reducer-less align -- every logged word within 1e-12
    (compare() at that tolerance), bit for bit where the two launches have the same descriptor (a reducer gives up the
    one-block-per-unit LDS padding of single-pose launches; batched launches keep their plan) -- and the hook is called
    once per launch-backed evaluation: ndt_result::n_evaluations counts exactly those (NewtonMachine::ask raises it only
    when it launches; requests answered from the memo count in n_evaluations_reused alone), which the evaluation log
    confirms independently; K calls for a batch of K."""
    from test_gpu_launch_shapes import compare
    cfg, ndt = _small(pkg, S)
    try:
        T0, r0, b0, log0, na0 = _logged_run(ndt, cfg)
        calls = []

        def ident(_ctx, words_p, n):
            calls.append(n)
            return 0

        ndt.commInitHook(ident, 0, 1)
        assert ndt.commRankCount() == 1
        T1, r1, b1, log1, na1 = _logged_run(ndt, cfg)
        assert calls == [32] * len(log1) and na1 == r1["n_evaluations"] and len(log1) == na1 + 3
        print("\nhook world 1: %d launches, %d reused" % (r1["n_evaluations"], r1["n_evaluations_reused"]))
        assert len(log1) == len(log0) and r1["iterations"] == r0["iterations"]
        gscale = max(np.linalg.norm(pkg.unpack_eval(e["words"])["gradient"]) for e in log0)
        same_desc = 0
        for i, (a, b) in enumerate(zip(log1, log0)):
            compare(pkg.unpack_eval(a["words"]), pkg.unpack_eval(b["words"]), gscale, True, ("hook vs none", i), tol=1e-12)
            if a["desc"] == b["desc"] and np.array_equal(bits(a["pose6"]), bits(b["pose6"])) and np.array_equal(a["T32"], b["T32"]):
                assert np.array_equal(bits(a["words"]), bits(b["words"])), ("same descriptor", i)
                same_desc += 1
        assert np.array_equal(bits(log1[0]["pose6"]), bits(log0[0]["pose6"]))
        print("  %d of %d evaluations with the reducer-less launch descriptor: bit-identical" % (same_desc, len(log1)))
    finally:
        ndt.close()


def test_hook_failure_and_argument_errors(pkg, S, refs):
    """A hook that reports failure: align and evalDerivatives raise NDT_ERR_COMM (-8); after commDestroy the handle aligns
    to the bits it gave before.  ndt_comm_init_hook refuses a NULL function, rank >= nranks and nranks < 1 with -1."""
    import ctypes as C
    cfg, ndt = _small(pkg, S)
    try:
        T0 = ndt.align(cfg["guess"])
        r0 = ndt.getResult()
        ndt.commInitHook(lambda _ctx, _w, _n: 1, 0, 1)
        with pytest.raises(pkg.NdtError) as ei:
            ndt.align(cfg["guess"])
        assert ei.value.code == -8
        with pytest.raises(pkg.NdtError) as ei:
            ndt.evalDerivatives(r0["pose"])
        assert ei.value.code == -8
        ndt.commDestroy()
        T1 = ndt.align(cfg["guess"])
        r1 = ndt.getResult()
        assert np.array_equal(bits(T1), bits(T0)) and np.array_equal(bits(r1["hessian"]), bits(r0["hessian"]))
        assert r1["iterations"] == r0["iterations"] and r1["n_evaluations"] == r0["n_evaluations"]
        for rank, nranks in ((1, 1), (2, 2), (0, 0), (0, -1), (-1, 2)):
            with pytest.raises(pkg.NdtError) as ei:
                ndt.commInitHook(lambda _ctx, _w, _n: 0, rank, nranks)
            assert ei.value.code == -1, (rank, nranks)
        assert pkg.lib().ndt_comm_init_hook(ndt._h, pkg.ALLREDUCE_FN(), None, 0, 1) == -1   # (a NULL function pointer)
        assert ndt.commRankCount() == 1
        T2 = ndt.align(cfg["guess"])
        assert np.array_equal(bits(T2), bits(T0))
    finally:
        ndt.close()


def test_reducer_reinitialised_on_one_handle(pkg, S, refs):
    """commDestroy, then another reducer on the same handle, several times over (shm, hook, shm again under the same
    name): every align gives the same bits as the first one under a reducer (the round counters restart with every init),
    and the reducer-less align's pose."""
    cfg, ndt = _small(pkg, S)
    name = "/ndt_reinit_%d" % os.getpid()
    try:
        Tn = ndt.align(cfg["guess"])
        got = []
        for kind in ("shm", "hook", "shm", "hook"):
            if kind == "shm":
                ndt.commInitShm(name, 0, 1)
            else:
                ndt.commInitHook(lambda _ctx, _w, _n: 0, 0, 1)
            assert ndt.commRankCount() == 1
            T = ndt.align(cfg["guess"])
            r = ndt.getResult()
            sc = ndt.scoreTransform(T)
            got.append((T, r["hessian"], r["iterations"], r["n_evaluations"], sc["score"]))
            ndt.commDestroy()
            assert ndt.commRankCount() == 1
        for g in got[1:]:
            assert np.array_equal(bits(g[0]), bits(got[0][0])) and np.array_equal(bits(g[1]), bits(got[0][1]))
            assert g[2:] == got[0][2:]
        dt, dr = S.pose_error(got[0][0], Tn)
        assert dt < 1e-5 and dr < 1e-6   # (the bounds of test_two_processes_one_gpu_shm_reduction)
        assert np.array_equal(bits(ndt.align(cfg["guess"])), bits(Tn))
    finally:
        ndt.close()
