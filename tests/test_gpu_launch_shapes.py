"""k_derivatives at every launch shape and path, word by word against the oracle.

The derivative kernel runs in many arrangements: 64 .. 1024 threads per block (1 .. 16 waves and the finishing-wave tables
of each), 0 / 1 / 4 summing blocks or the doubling split, XCD-aware chunk order, one or several residency rounds, the
two-level final sum, and the template axes <BATCH, MODE, NB, MBOX>.  The end-to-end tests see most of them only through
an align's final pose.  Here the engine's evaluation log (ndt_debug_eval_log, a test seam of the production library)
records every evaluation a launch made -- pose and f32 transform in, the raw 32 words out (before the ridge /
regularisation of finish_eval), and the launch's plan -- and each one is compared with the oracle's f64 statement of
the same evaluation (pair_mode 2: what the kernel computes):
  * n_pairs and n_with_neighbors exactly; score, NVTL sum and Hessian within 1e-9 relative; the gradient within 1e-9 of the largest
    gradient norm of the evaluations compared together (its norm falls by ~1e4 along a trajectory while its terms do
    not, as in test_gpu_trajectory.py); packed 48-byte records within test_packed_voxel_records' bounds;
  * the plan of the launch the engine made is the host plan for that size (ndt_debug_launch_plan);
  * what is promised bit for bit is compared bit for bit: single-pose against batched K = 1, pre-launched against
    ordinary, batched K > 1 against K = 1 where the partition is the same.

Sources are the simulated C3 scan (261 907 points; S.config_c3(n_src=n)'s source is this scan subsampled in order, the
same points), and above that jittered copies of it, as test_large_source_two_level_final_sum makes them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULL_SCAN = 261907
KW = dict(resolution=0.5, step_size=0.1, trans_epsilon=1e-4)
TOL = 1e-9

# n -> what it covers (single-pose shape on a whole MI355X, 256 compute units; tests/test_abi_cpu.py pins these plans)
SHAPES = {
    20000: "4 waves, 4 summing blocks",
    55000: "5 waves",
    70000: "6 waves",
    80000: "7 waves",
    95000: "8 waves (small-source partition)",
    130000: "8 waves, one summing block",
    131072: "8 waves, no unit spare: doubling split",
    140000: "9 waves",
    155000: "10 waves",
    170000: "11 waves",
    190000: "12 waves",
    200000: "13 waves (C3)",
    220000: "14 waves",
    235000: "15 waves",
    250000: "16 waves",
    261000: "16 waves, one summing block",
    400000: "several residency rounds",
    1200000: "two-level final sum",
}


def c3_source(full, n):
    if n == len(full):
        return full
    if n < len(full):
        return full[np.sort(np.random.default_rng(11).choice(len(full), size=n, replace=False))]
    rng = np.random.default_rng(5)
    reps = -(-n // len(full))
    return np.concatenate([full] + [(full + rng.normal(0, 0.01, full.shape)).astype(np.float32)
                                    for _ in range(reps - 1)])[:n]


class Ctx:
    def __init__(self, pkg, O, S):
        self.pkg, self.O, self.S = pkg, O, S
        self.cfg = S.config_c3(n_src=FULL_SCAN)
        assert len(self.cfg["source"]) == FULL_SCAN
        self.prm = O.default_params(num_threads=16, pair_mode=2, max_iterations=3, **KW)
        self.grid = O.Grid(self.cfg["target"], self.prm)
        self.ndt = pkg.NormalDistributionsTransform(device_id=0, max_iterations=3, **KW)
        self.ndt.setInputTarget(self.cfg["target"])
        self.ndt.wait()
        self.sources = {}
        self.grids = {}
        self.memo = {}
        self.worst = {}          # shape class -> worst relative error against the oracle {score, g, H}
        self.ledger = {}         # (BATCH, MODE, NB, MBOX) -> evaluations compared with the oracle

    def source(self, n):
        if n not in self.sources:
            self.sources = {n: c3_source(self.cfg["source"], n)}   # (one at a time: 1.2 M points are 14 MB)
        return self.sources[n]

    def oracle(self, n, e, prm=None, key=None):
        k = (n, key, e["pose6"].tobytes(), e["T32"].tobytes(), e["need_h"])
        if k not in self.memo:
            self.memo[k] = self.grid.derivatives(self.source(n), e["pose6"], T=e["T"], compute_hessian=e["need_h"],
                                                 params=prm or self.prm)
        return self.memo[k]

    def guesses(self):
        """the guess, the guess moved a little, ground truth"""
        g = self.cfg["guess"]
        return [g, g @ self.S.pose_matrix(0.05, -0.04, 0.02, 0.004, -0.003, 0.01), self.cfg["gt"]]

    def ogrid(self, omethod, tiles=None):
        """the oracle's grids of the map (or of the tiles of a multi-grid union) for one neighbourhood"""
        k = (omethod, tiles is not None)
        if k not in self.grids:
            prm = self.O.default_params(num_threads=16, pair_mode=2, max_iterations=3, search_method=omethod, **KW)
            self.grids[k] = [self.O.Grid(x, prm) for x in (tiles if tiles is not None else [self.cfg["target"]])]
        return self.grids[k]


@pytest.fixture(scope="module")
def ctx(pkg, O, S):
    n, info = pkg.backend_info()
    assert n > 0, "GPU test on a box without a HIP device: " + info
    c = Ctx(pkg, O, S)
    yield c
    c.ndt.close()


def words_of(pkg, e):
    return pkg.unpack_eval(e["words"])


def compare(got, d, gscale, need_h, what, tol=TOL, worst=None):
    """got: unpacked kernel words; d: the oracle's.  Returns nothing; records the worst relative errors."""
    assert got["n_pairs"] == d["n_pairs"], (what, got["n_pairs"], d["n_pairs"])
    if d["n_with_neighbors"] is not None:
        assert got["n_with_neighbors"] == d["n_with_neighbors"], (what, got["n_with_neighbors"], d["n_with_neighbors"])
        assert abs(got["nvtl_sum"] - d["nvtl_sum"]) <= tol * abs(d["nvtl_sum"]) + 1e-9, (what, got["nvtl_sum"], d["nvtl_sum"])
    es = abs(got["score"] - d["score"]) / abs(d["score"])
    eg = np.linalg.norm(got["gradient"] - d["gradient"]) / gscale
    eh = np.linalg.norm(got["hessian"] - d["hessian"]) / np.linalg.norm(d["hessian"]) if need_h else 0.0
    if worst is not None:
        for k, v in (("score", es), ("g", eg), ("H", eh)):
            worst[k] = max(worst.get(k, 0.0), v)
    assert es < tol and eg < tol and eh < tol, (what, es, eg, eh)


def bits(w):
    return np.ascontiguousarray(w, dtype=np.float64).view(np.uint64)


def check_plan(pkg, n, e, what):
    d = dict(e["desc"])
    assert d["safe_sum"] == 0, (what, "a ticketed re-evaluation: a summing block gave up waiting for a row", d)
    want = pkg.debug_launch_plan(n, K=e["K"], cus=d["cus"], nb=d["nb"], mode=d["mode"], batched=bool(d["batch"]),
                                 mbox=bool(d["mbox"]))
    assert {k: v for k, v in d.items() if k != "spec"} == {k: v for k, v in want.items() if k != "spec"}, (what, d, want)
    t, pb, ns, grid = pkg.debug_launch_shape(n, e["K"], d["cus"])
    assert (d["threads"], d["point_blocks"], d["summers"], d["blocks"]) == (t, pb, ns, grid), (what, d)


def aligns_with_log(ctx, prelaunch):
    """the three aligns of a shape with the evaluation log on: [(log, result)]"""
    ndt, pkg = ctx.ndt, ctx.pkg
    ndt.setParams(prelaunch=prelaunch)
    out = []
    for g in ctx.guesses():
        ndt.debugEvalLog(512)
        T = ndt.align(g)
        log = ndt.debugEvalLogRead()
        out.append((log, T, ndt.getResult()))
    ndt.debugEvalLog(0)
    return out


def record(ctx, e):
    d = e["desc"]
    key = (d["batch"], d["mode"], d["nb"], d["mbox"])
    ctx.ledger[key] = ctx.ledger.get(key, 0) + 1


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_single_pose_and_batched_at_every_shape(ctx, n):
    """Single-pose kernel (ordinary first evaluation, speculative, pre-launched) through align, batched K = 1 at the
    same poses, pre-launch on / off, batched K = 2 / 7 / 20 -- against the oracle and each other."""
    pkg, ndt = ctx.pkg, ctx.ndt
    src = ctx.source(n)
    ndt.setInputSource(src)
    worst = ctx.worst.setdefault(SHAPES[n], {})
    used0 = ndt.prelaunchCounters()[0]
    on = aligns_with_log(ctx, pkg.PRELAUNCH_AUTO)
    used = ndt.prelaunchCounters()[0] - used0
    off = aligns_with_log(ctx, pkg.PRELAUNCH_OFF)
    ndt.setParams(prelaunch=pkg.PRELAUNCH_AUTO)
    entries = [e for log, _, _ in on for e in log]
    assert entries and all(e["K"] == 1 and e["desc"]["batch"] == 0 and e["need_h"] for e in entries)
    gscale = max(np.linalg.norm(ctx.oracle(n, e)["gradient"]) for e in entries)
    n_pre = 0
    for i, e in enumerate(entries):
        what = (n, i, "prelaunched" if e["prelaunched"] else "ordinary")
        check_plan(pkg, n, e, what)
        assert e["desc"]["mbox"] == int(e["prelaunched"])
        n_pre += e["prelaunched"]
        compare(words_of(pkg, e), ctx.oracle(n, e), gscale, True, what, worst=worst)
        record(ctx, e)
    assert n_pre == used
    # pre-launched evaluations are the ordinary ones, bit for bit (same poses, same words, same aligns)
    for (la, Ta, ra), (lb, Tb, rb) in zip(on, off):
        assert np.array_equal(Ta, Tb) and ra["iterations"] == rb["iterations"] and np.array_equal(ra["hessian"], rb["hessian"])
        assert len(la) == len(lb)
        for a, b in zip(la, lb):
            assert not b["prelaunched"] and np.array_equal(bits(a["pose6"]), bits(b["pose6"]))
            assert np.array_equal(bits(a["words"]), bits(b["words"])), (n, a["prelaunched"])
    # the single-pose kernel and the batched one of one pose: the same 32 words
    distinct = {}
    for e in entries:
        distinct.setdefault((e["pose6"].tobytes(), e["T32"].tobytes()), e)
    singles = list(distinct.values())
    ndt.debugEvalLog(len(singles))
    for e in singles:
        ndt.evalDerivatives(e["pose6"], transforms=[e["T"]])
    batched1 = ndt.debugEvalLogRead()
    for e, b in zip(singles, batched1):
        assert b["desc"]["batch"] == 1 and b["K"] == 1
        check_plan(pkg, n, b, (n, "K=1"))
        record(ctx, b)
        assert np.array_equal(bits(e["words"]), bits(b["words"])), (n, "single-pose != batched K = 1")
    # batched K > 1: every pose against the oracle; against K = 1 bit for bit where the partition is the same
    rng = np.random.default_rng(n)
    poses = [e["pose6"] for e in singles]
    while len(poses) < 20:
        poses.append(poses[len(poses) % len(singles)] + rng.normal(0, [0.02, 0.02, 0.01, 0.002, 0.002, 0.005]))
    poses = np.stack(poses[:20])
    ndt.debugEvalLog(20)
    for p in poses:
        ndt.evalDerivatives(p)
    one = ndt.debugEvalLogRead()
    for K in (2, 7, 20):
        # derivs_block_threads keeps the K = 1 partition for every K up to 196 x 512 points and wherever the single-pose
        # shape is the 512-thread one (131 072, and the grids of several residency rounds); the 9 .. 16-wave single-pose
        # blocks of 131 k .. 261 k points are a single-pose shape only
        same_partition = pkg.debug_launch_shape(n, K)[0] == pkg.debug_launch_shape(n, 1)[0]
        assert same_partition or 131072 < n <= 261120
        ndt.debugEvalLog(K)
        ndt.evalDerivatives(poses[:K])
        got = ndt.debugEvalLogRead()
        assert len(got) == K
        gK = max(np.linalg.norm(ctx.oracle(n, e)["gradient"]) for e in got)
        for k, (e, s) in enumerate(zip(got, one)):
            assert e["K"] == K and e["k"] == k and np.array_equal(e["T32"], s["T32"])
            check_plan(pkg, n, e, (n, K, k))
            record(ctx, e)
            compare(words_of(pkg, e), ctx.oracle(n, e), gK, True, (n, K, k), worst=worst)
            if same_partition:
                assert np.array_equal(bits(e["words"]), bits(s["words"])), (n, K, k)
            else:
                # another block shape (single-pose 9 .. 16-wave blocks, batched 512): the same sums over another
                # partition -- the last bits of an f64 sum of ~1e5 terms, far below the oracle bound
                compare(words_of(pkg, e), words_of(pkg, s), gK, True, (n, K, k, "vs K=1"), tol=1e-12)
    ndt.debugEvalLog(0)


# neighbourhoods: (engine search method, record format, oracle search method, NB template value)
def _nbs(pkg, O):
    return [(pkg.DIRECT1, pkg.RECORDS_F64, O.DIRECT1, 0), (pkg.DIRECT7, pkg.RECORDS_F64, O.DIRECT7, 1),
            (pkg.KDTREE, pkg.RECORDS_F64, O.KDTREE, 2), (pkg.DIRECT26, pkg.RECORDS_F64, O.DIRECT26, 3),
            (pkg.DIRECT1, pkg.RECORDS_PACKED48, O.DIRECT1, 5), (pkg.DIRECT7, pkg.RECORDS_PACKED48, O.DIRECT7, 6)]


def _modes_matrix(ctx, n, multigrid_ok=True):
    """every neighbourhood x Hessian kind x entry point at one size, each evaluation against the oracle"""
    pkg, O, S = ctx.pkg, ctx.O, ctx.S
    src = ctx.source(n)
    worst = ctx.worst.setdefault("modes %d" % n, {})
    guess = ctx.cfg["guess"]
    p_guess, p_gt = O.matrix_to_pose(guess), O.matrix_to_pose(ctx.cfg["gt"])
    poses, Ts = np.stack([p_guess, p_gt]), [guess, ctx.cfg["gt"]]
    cases = [(m, f, om, nb, None) for m, f, om, nb in _nbs(pkg, O)]
    if multigrid_ok:
        cases.append((None, pkg.RECORDS_F64, O.KDTREE, 4, "multigrid"))
    t = ctx.cfg["target"]
    cut = float(np.median(t[:, 0]))
    tiles = (t[t[:, 0] <= cut + 2.0], t[t[:, 0] >= cut - 2.0])   # two grids that share the voxels of a 4 m strip
    for method, fmt, omethod, nb, kind in cases:
        for hmode in (pkg.HESSIAN_FULL, pkg.HESSIAN_GAUSS_NEWTON):
            oprm = O.default_params(num_threads=16, pair_mode=2, max_iterations=3, search_method=omethod,
                                    hessian_mode=0 if hmode == pkg.HESSIAN_FULL else 1, **KW)
            ndt = pkg.NormalDistributionsTransform(device_id=0, max_iterations=3, hessian_mode=hmode, **KW)
            try:
                if kind == "multigrid":
                    grids = ctx.ogrid(omethod, tiles)
                    for i, x in enumerate(tiles):
                        ndt.addTarget(x, 10 + i)
                    ndt.createVoxelKdtree()
                else:
                    ndt.setParams(search_method=method)
                    ndt.setRecordFormat(fmt)
                    ndt.setInputTarget(t)
                    grids = ctx.ogrid(omethod)
                ndt.setInputSource(src)

                def oracle(e):
                    # (a union: score, gradient, Hessian and pairs are the sums of the grids' KDTREE evaluations; a point
                    # with neighbours in both grids counts once in n_with_neighbors, and its nvtl term is a maximum over
                    # all its neighbours -- neither is a sum, and the union's are not compared with the oracle)
                    ds = [g.derivatives(src, e["pose6"], T=e["T"], compute_hessian=e["need_h"], params=oprm) for g in grids]
                    one = len(ds) == 1
                    return dict(score=sum(d["score"] for d in ds), gradient=sum(d["gradient"] for d in ds),
                                hessian=sum(d["hessian"] for d in ds), n_pairs=sum(d["n_pairs"] for d in ds),
                                n_with_neighbors=ds[0]["n_with_neighbors"] if one else None,
                                nvtl_sum=ds[0]["nvtl_sum"] if one else None)

                ndt.debugEvalLog(512)
                ndt.align(guess)                                       # MODE 1 / 2, single-pose (+ pre-launched)
                ndt.evalDerivatives(poses, transforms=Ts)                          # batched, Hessian
                ndt.evalDerivatives(poses, transforms=Ts, compute_hessian=False)   # batched MODE 0
                sc1 = [ndt.scoreTransform(T) for T in Ts]                          # single-pose MODE 3
                scK = ndt.scoreTransforms(Ts)                                      # batched MODE 3
                log = ndt.debugEvalLogRead()
                ndt.debugEvalLog(0)
                want_mode = 1 if hmode == pkg.HESSIAN_FULL else 2
                gscale = max(np.linalg.norm(oracle(e)["gradient"]) for e in log if not e["score_only"])
                by_kind = {}
                for i, e in enumerate(log):
                    d = e["desc"]
                    what = (n, nb, hmode, i, d["batch"], d["mode"], d["mbox"])
                    assert d["nb"] == nb, what
                    assert d["mode"] == (3 if e["score_only"] else (want_mode if e["need_h"] else 0)), what
                    check_plan(ctx.pkg, n, e, what)
                    record(ctx, e)
                    got, ref = words_of(pkg, e), oracle(e)
                    by_kind.setdefault((d["batch"], d["mode"]), []).append(e)
                    if e["score_only"]:
                        assert got["n_pairs"] == ref["n_pairs"], what
                        assert ref["n_with_neighbors"] is None or got["n_with_neighbors"] == ref["n_with_neighbors"], what
                        tol = 1e-6 if nb in (5, 6) else TOL
                        assert abs(got["score"] - ref["score"]) <= tol * abs(ref["score"]), what
                        continue
                    if nb in (5, 6):
                        # packed records (test_packed_voxel_records): the inverse covariance rounded to f32
                        assert got["n_pairs"] == ref["n_pairs"], what
                        assert got["score"] == pytest.approx(ref["score"], rel=1e-6), what
                        assert np.linalg.norm(got["gradient"] - ref["gradient"]) <= 2e-6 * np.linalg.norm(ref["gradient"]) + 1e-9, what
                        continue
                    compare(got, ref, gscale, e["need_h"], what, worst=worst)
                # exact equalities between paths at the same pose: MODE 3 against MODE 1 (score, pairs, nvtl);
                # MODE 0's gradient against MODE 1's
                b1, b0, b3 = by_kind[(1, want_mode)], by_kind[(1, 0)], by_kind[(1, 3)]
                s3 = by_kind[(0, 3)]
                same_partition = pkg.debug_launch_shape(n, 2)[0] == pkg.debug_launch_shape(n, 1)[0]
                for x1, x0, x3, y3 in zip(b1, b0, b3, s3):
                    assert x1["words"][0] == x3["words"][0], (n, nb, "score MODE 3 vs 1")
                    assert np.array_equal(x1["words"][28:31], x3["words"][28:31]), (n, nb, "nvtl / counts MODE 3 vs 1")
                    # single-pose MODE 3 (scoreTransform) against the batched one: bit for bit on the same partition;
                    # elsewhere (single-pose 9 .. 16-wave blocks) the same sum over other blocks
                    assert np.array_equal(x3["words"][29:31], y3["words"][29:31]), (n, nb, "counts single vs batched")
                    if same_partition:
                        assert np.array_equal(bits(x3["words"][[0, 28]]), bits(y3["words"][[0, 28]])), (n, nb, "MODE 3 single vs batched")
                    else:
                        assert abs(x3["words"][0] - y3["words"][0]) <= 1e-12 * abs(x3["words"][0]), (n, nb)
                    if want_mode == 1:
                        assert np.array_equal(bits(x1["words"][1:7]), bits(x0["words"][1:7])), (n, nb, "g MODE 0 vs 1")
                for s, y3 in zip(sc1 + scK, s3 + b3):
                    assert s["score"] == y3["words"][0] and s["n_pairs"] == int(y3["words"][30])
            finally:
                ndt.close()


@pytest.mark.parametrize("n", [200000, 250000])
def test_modes_and_neighbourhoods(ctx, n):
    """Every neighbourhood (DIRECT1 / DIRECT7 / KDTREE / DIRECT26 / multi-grid, packed DIRECT1 / DIRECT7) with the full
    and the Gauss-Newton Hessian, through align, evalDerivatives with and without the Hessian, scoreTransform and
    scoreTransforms, at the 13-wave C3 shape and a 16-wave one (the 256-thread shape: the ledger test)."""
    _modes_matrix(ctx, n)


# the instantiations no entry point reaches: align always asks for the Hessian (newton_align with hessian_in_trials,
# ndt_newton.cpp), so the single-pose kernel never runs MODE 0; a pre-launched kernel is armed only inside align
# (prelaunch needs !score_only), so MBOX = true never runs MODE 0 or 3; a batched launch never takes the mailbox
DEAD = sorted([(0, 0, nb, mb) for nb in range(7) for mb in (0, 1)] + [(0, 3, nb, 1) for nb in range(7)] +
              [(1, m, nb, 1) for m in range(4) for nb in range(7)])


def test_instantiation_ledger(ctx):
    """The 256-thread shape (20 k points) through the whole matrix of neighbourhoods, Hessians and entry points, and the
    ledger of the instantiations <BATCH, MODE, NB, MBOX> whose evaluations were compared with the oracle in this module
    (this test's own matrix reaches every live one, whatever ran before it).  Of the 2 x 4 x 7 x 2 = 112 combinations
    the 28 batched MBOX ones are never compiled (launch_derivatives takes the mailbox only for single-pose launches),
    leaving the 84 instantiations; of those 21 are unreachable: <false, 0, *, false> (align always asks for the
    Hessian) and <false, {0, 3}, *, true> (pre-launch needs an align) -- 63 are live."""
    _modes_matrix(ctx, 20000)
    live = sorted({(b, m, nb, mb) for b in (0, 1) for m in range(4) for nb in range(7) for mb in (0, 1)} - set(DEAD))
    assert len(live) == 63 and len(DEAD) - 28 == 21
    mbox_seen = any(k[3] == 1 for k in ctx.ledger)
    missing = [k for k in live if k not in ctx.ledger and (k[3] == 0 or mbox_seen)]
    assert not missing, missing
    assert not [k for k in ctx.ledger if k in DEAD], [k for k in ctx.ledger if k in DEAD]
    print("\ninstantiations compared with the oracle: %d of %d live%s" %
          (len([k for k in live if k in ctx.ledger]), len(live), "" if mbox_seen else " (no BAR-mapped memory: MBOX ones not run)"))
    for k in live:
        print("  <%s, %d, %d, %s>: %d evaluations" % ("true" if k[0] else "false", k[1], k[2], "true" if k[3] else "false",
                                                     ctx.ledger.get(k, 0)))
    for cls, w in ctx.worst.items():
        print("  worst vs oracle, %-40s score %.1e  g %.1e  H %.1e" % (cls, w.get("score", 0), w.get("g", 0), w.get("H", 0)))


# ndt_tuning fields: non-default valid values.  Bit-neutral ones (include/ndt_hip.h): every word equals the defaults'
NEUTRAL = [("deriv_summer", 0), ("deriv_dedicated", 0), ("deriv_xcd", 0), ("deriv_xcd", 2), ("deriv_one_block_per_cu", 0),
           ("deriv_summer_split", 0), ("deriv_summer_split", 8), ("mbox_tagged", 0), ("mbox_preload", 1),
           ("prelaunch_streams", 1), ("prelaunch_probe", 0), ("speculate_first", 0), ("timing_bracket", 1),
           ("bounds_blocks", 64), ("bounds_unroll", 4), ("finalize_threads", 64), ("build_events", 0), ("build_events", 1),
           ("build_wait_sync", 1), ("bucket_build", 0), ("bucket_tile", 1024), ("bucket_tile", 8192), ("fused_sort", 0),
           ("handoff_chunk_pass", 1)]
PARTITION = [("deriv_block", v) for v in (64, 128, 192, 320, 576, 1024)] + [("deriv_single_level_max", v) for v in (1, 8, 64)]


def _tuned_run(pkg, cfg, res, timing):
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=res, step_size=0.1, trans_epsilon=1e-4, max_iterations=5)
    try:
        if timing:
            ndt.enableKernelTiming(True)
        ndt.debugEvalLog(512)
        ndt.setInputTarget(cfg["target"])
        ndt.setInputSource(cfg["source"])
        T = ndt.align(cfg["guess"])
        r = ndt.getResult()
        ndt.evalDerivatives(np.stack([r["pose"], np.zeros(6)]))
        log = ndt.debugEvalLogRead()
        leaves = ndt.getLeaves()
        return dict(T=T, it=r["iterations"], nev=r["n_evaluations"], H=r["hessian"], log=log, leaves=leaves)
    finally:
        ndt.close()


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_tuning_promises(ctx, name):
    """Every ndt_tuning field at each non-default valid value on a fresh handle: the fields include/ndt_hip.h calls
    result-neutral change no bit of the align (transform, iterations, evaluations, final Hessian), of any logged word,
    or of the exported leaves; deriv_block (1 .. 16 waves) and deriv_single_level_max (two-level sums over few rows)
    change the partition and stay within 1e-9 of the oracle and 1e-12 of the defaults' evaluation at the same pose."""
    pkg, O, S = ctx.pkg, ctx.O, ctx.S
    if name == "c2":
        cfg, res = S.config_c2(), 1.0
    else:
        cfg, res = dict(ctx.cfg, source=ctx.source(200000)), 0.5
    prm = O.default_params(num_threads=16, pair_mode=2, max_iterations=5, resolution=res, step_size=0.1, trans_epsilon=1e-4)
    grid = O.Grid(cfg["target"], prm) if name == "c2" else ctx.grid
    before = pkg.get_tuning()
    try:
        base = {tm: _tuned_run(pkg, cfg, res, tm) for tm in (False, True)}
        for field, value in NEUTRAL:
            pkg.set_tuning(**before)
            pkg.set_tuning(**{field: value})
            timing = field == "timing_bracket"
            got, ref = _tuned_run(pkg, cfg, res, timing), base[timing]
            what = (name, field, value)
            assert np.array_equal(got["T"], ref["T"]) and got["it"] == ref["it"] and got["nev"] == ref["nev"], what
            assert np.array_equal(got["H"], ref["H"]), what
            assert len(got["log"]) == len(ref["log"]), what
            for a, b in zip(got["log"], ref["log"]):
                assert np.array_equal(bits(a["pose6"]), bits(b["pose6"])), what
                assert np.array_equal(bits(a["words"]), bits(b["words"])), what
            for k in ("cell", "count", "mean", "cov", "icov"):
                assert np.array_equal(got["leaves"][k], ref["leaves"][k]), (what, k)
        ref = base[False]
        for field, value in PARTITION:
            pkg.set_tuning(**before)
            pkg.set_tuning(**{field: value})
            got = _tuned_run(pkg, cfg, res, False)
            what = (name, field, value)
            gscale = max(np.linalg.norm(grid.derivatives(cfg["source"], e["pose6"], T=e["T"], params=prm)["gradient"])
                         for e in got["log"])
            n = len(cfg["source"])
            for e in got["log"]:
                d = e["desc"]
                if field == "deriv_block":
                    assert d["threads"] == value, what
                else:
                    assert d["two_level"] == (d["point_blocks"] > value), what
                check_plan(pkg, n, e, what)
                oref = grid.derivatives(cfg["source"], e["pose6"], T=e["T"], compute_hessian=e["need_h"], params=prm)
                compare(words_of(pkg, e), oref, gscale, e["need_h"], what,
                        worst=ctx.worst.setdefault("tuning %s %s" % (name, field), {}))
            # the same poses as the defaults' run: within 1e-12 of its words
            same = 0
            for a, b in zip(got["log"], ref["log"]):
                if np.array_equal(bits(a["pose6"]), bits(b["pose6"])) and a["need_h"] == b["need_h"]:
                    compare(words_of(pkg, a), words_of(pkg, b), gscale, a["need_h"], what + ("vs default",), tol=1e-12)
                    same += 1
            assert same >= 1, what
    finally:
        pkg.set_tuning(**before)
