"""CPU tests of the multi-hypothesis driver (ndt_newton_align_batch; no GPU): K Newton / More-Thuente loops advanced in
lockstep with the CPU oracle as a batched evaluator give, hypothesis for hypothesis, the bits newton_align gives from
the same guess, and every round hands the evaluator exactly the pending requests of the loops still running."""
import ctypes as C

import numpy as np
import pytest

KW = dict(resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=35)
FIELDS = ("T", "pose", "hessian", "score", "iterations", "n_evaluations", "n_evaluations_reused", "converged",
          "transform_probability", "nvtl", "n_pairs", "n_points_with_neighbors")


def _guesses(S, cfg):
    g = cfg["guess"]
    return [g,
            g @ S.pose_matrix(0.3, -0.3, 0.1, 0.02, -0.03, 0.05),
            cfg["gt"],
            g @ S.pose_matrix(-0.3, 0.3, 0.0, 0.0, 0.0, -0.052),
            g @ S.pose_matrix(1.5, -1.0, 0.2, 0.0, 0.0, 0.3)]   # runs into max_iterations


class _Oracle:
    """The oracle's derivatives as packed words, memoised on (pose, T, need_h): a pure function of its request, so
    the serial and the batched runs can share evaluations without changing a bit."""

    def __init__(self, pkg, O, cfg):
        self.pkg = pkg
        self.prm = O.default_params(symmetrize_hessian=1, **KW)
        self.grid = O.Grid(cfg["target"], self.prm)
        self.src = cfg["source"]
        self.cache = {}

    def __call__(self, pose, T, need_h):
        key = (np.asarray(pose, np.float64).tobytes(), np.asarray(T, np.float32).tobytes(), bool(need_h))
        if key not in self.cache:
            d = self.grid.derivatives(self.src, pose, T=T, compute_hessian=bool(need_h), params=self.prm)
            self.cache[key] = self.pkg.pack_eval(d["score"], d["gradient"], d["hessian"], d["nvtl_sum"],
                                                 d["n_with_neighbors"], d["n_pairs"])
        return self.cache[key]


@pytest.fixture(scope="module", params=["c1", "c2"])
def case(request, pkg, O, S):
    cfg = getattr(S, "config_" + request.param)()
    return cfg, _Oracle(pkg, O, cfg)


@pytest.mark.parametrize("regularized", [False, True])
def test_batch_reproduces_serial_newton_align(pkg, S, case, regularized):
    cfg, ev = case
    n = len(cfg["source"])
    guesses = _guesses(S, cfg)
    reg = S.pose_matrix(0.45, 0.02, 0.3, 0.0, 0.0, 0.26) @ cfg["gt"] if regularized else None
    kw = dict(KW, regularization_scale_factor=0.01) if regularized else KW
    serial, logs = [], []
    for G in guesses:
        log = []

        def logged(pose, T, need_h, log=log):
            log.append((np.array(pose), np.asarray(T, np.float32).copy(), bool(need_h)))
            return ev(pose, T, need_h)
        serial.append(pkg.newton_align(pkg.default_params(**kw), n, G, logged, regularization_pose=reg))
        logs.append(log)
    rounds = []

    def batch_ev(poses, Ts, need):
        rounds.append((poses.copy(), np.asarray(Ts, np.float32).copy(), need.copy()))
        return np.stack([ev(poses[i], Ts[i], need[i]) for i in range(len(poses))])
    got = pkg.newton_align_batch(pkg.default_params(**kw), n, guesses, batch_ev, regularization_pose=reg)
    assert len(got) == len(guesses)
    for k, (a, b) in enumerate(zip(got, serial)):
        for f in FIELDS:
            assert np.array_equal(a[f], b[f]), (k, f, a[f], b[f])
        assert a["n_evaluations"] == len(logs[k])
    assert any(r["iterations"] == KW["max_iterations"] + 2 for r in serial)   # one loop stops at the iteration cap
    assert len({r["iterations"] for r in serial}) > 2                         # loops of different lengths share rounds
    # every round carries exactly the pending request of each loop still running, in hypothesis order
    assert len(rounds) == max(len(lg) for lg in logs)
    for r, (poses, Ts, need) in enumerate(rounds):
        live = [k for k in range(len(guesses)) if len(logs[k]) > r]
        assert len(poses) == len(live)
        for i, k in enumerate(live):
            p, T, h = logs[k][r]
            assert np.array_equal(poses[i], p) and np.array_equal(Ts[i], T) and bool(need[i]) == h


def test_batch_of_one_is_newton_align(pkg, S):
    src, tgt, gt, guess = S.two_planes(seed=3, max_points=1500)
    calls = []

    def ev(pose, T, need_h):   # a smooth concave stand-in: the driver only needs consistent words
        d = np.asarray(pose) - np.array([0.2, -0.1, 0.05, 0.01, 0.0, 0.03])
        calls.append(1)
        return pkg.pack_eval(-float(d @ d) * 1000.0, -2000.0 * d, -2000.0 * np.eye(6), 1.0, 1, 1)
    a = pkg.newton_align(pkg.default_params(**KW), len(src), guess, ev)
    b = pkg.newton_align_batch(pkg.default_params(**KW), len(src), [guess],
                               lambda P, T, h: np.stack([ev(P[i], T[i], h[i]) for i in range(len(P))]))[0]
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), f


def test_argument_errors(pkg, S):
    L = pkg.lib()
    prm = pkg.default_params(**KW)
    res = (pkg.Result * 2)()
    g = np.ascontiguousarray(np.tile(np.eye(4, dtype=np.float32).ravel(), 300))
    gp = g.ctypes.data_as(C.POINTER(C.c_float))
    called = []
    cb = pkg.EVAL_BATCH_FN(lambda *a: called.append(1) or -1)
    for K in (0, -1, 257):
        assert L.ndt_newton_align_batch(C.byref(prm), 100, gp, K, None, cb, None, res) == -1
        assert L.ndt_align_batch(None, gp, K, res) == -1
    assert L.ndt_newton_align_batch(None, 100, gp, 1, None, cb, None, res) == -1
    assert L.ndt_newton_align_batch(C.byref(prm), 100, None, 1, None, cb, None, res) == -1
    assert L.ndt_newton_align_batch(C.byref(prm), 100, gp, 1, None, pkg.EVAL_BATCH_FN(), None, res) == -1
    assert L.ndt_newton_align_batch(C.byref(prm), 100, gp, 1, None, cb, None, None) == -1
    assert L.ndt_align_batch(None, gp, 1, res) == -1
    assert not called
    # the largest batch is accepted, and an evaluator's failure comes back as its code
    assert L.ndt_newton_align_batch(C.byref(prm), 100, gp, 256, None, cb, None, (pkg.Result * 256)()) == -1
    assert called == [1]
    with pytest.raises(pkg.NdtError):
        pkg.newton_align_batch(prm, 100, [], lambda *a: None)
    with pytest.raises(pkg.NdtError):
        pkg.newton_align_batch(prm, 100, [np.eye(4)] * 257, lambda *a: None)

    def boom(poses, T, need):
        raise RuntimeError("evaluator failed")
    with pytest.raises(pkg.NdtError):
        pkg.newton_align_batch(prm, 100, [np.eye(4)] * 3, boom)
