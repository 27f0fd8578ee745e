"""CPU companion of tests/test_gpu_sharded.py: its layout generator, its rank-ordered sum and its numpy restatement of
finish_eval, none of which needs a GPU."""
import math

import numpy as np
import pytest

from test_gpu_sharded import LAYOUTS, bits, finish_eval_np, layout_shards, rank_ordered_sum, sampled, shard_bounds

C2_POINTS, C3_POINTS = 128 * 1024, 200000


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layouts_are_contiguous_and_cover_the_source(pkg, name):
    wl, world, _ = LAYOUTS[name]
    n = C2_POINTS if wl == "c2" else C3_POINTS
    sizes = layout_shards(name, n, pkg.shard_range)
    assert len(sizes) == world and 3 <= world <= 7 and all(s >= 0 for s in sizes) and sum(sizes) == n
    at = 0
    for b, c in shard_bounds(sizes):
        assert b == at
        at += c
    assert at == n
    if name.startswith("even"):
        assert max(sizes) - min(sizes) <= 1 and [pkg.shard_range(n, r, world)[1] for r in range(world)] == sizes


def test_layouts_hold_the_sizes_they_claim(pkg):
    ragged = layout_shards("ragged6", C2_POINTS, pkg.shard_range)
    assert ragged[:5] == [0, 1, 63, 64, 65] and ragged[5] == C2_POINTS - 193
    assert layout_shards("lonely3", C2_POINTS, pkg.shard_range) == [0, C2_POINTS, 0]
    big = layout_shards("c3big3", C3_POINTS, pkg.shard_range)
    assert big == [150000, 50000, 0] and big[0] > 131072
    assert layout_shards("even7", C2_POINTS, pkg.shard_range).count(18724) == 3
    # the launch shapes that meet in one exchange: one wave's worth of points beside 8 waves, 9 .. 16 beside 4
    assert pkg.debug_launch_shape(65, 1)[1] == 1 and pkg.debug_launch_shape(ragged[5], 1)[0] == 512
    assert pkg.debug_launch_shape(150000, 1)[0] > 512 and pkg.debug_launch_shape(150000, 2)[0] == 512
    assert pkg.debug_launch_shape(50000, 1)[0] == 256
    assert pkg.debug_launch_shape(0, 1)[:2] == (256, 1)       # an empty shard: one block, nothing to read


def test_sampled_batch_indices():
    assert sampled(1) == [0] and sampled(5) == [0, 4] and sampled(20) == [0, 19]
    assert sampled(70) == [0, 63, 64, 69] and sampled(130) == [0, 63, 64, 127, 128, 129]


def test_rank_ordered_sum_is_the_left_to_right_sum():
    rows = np.array([[1e16, 0.5], [1.0, 0.25], [-1e16, 0.125]])
    s = rank_ordered_sum(rows)
    assert s[0] == 0.0 and s[1] == 0.875                     # (1e16 + 1) rounds to 1e16: the 1 is lost in rank order ...
    assert rank_ordered_sum(rows[[0, 2, 1]])[0] == 1.0       # ... and kept when the large terms cancel first
    assert math.fsum(rows[:, 0]) == 1.0 != s[0]              # (the exact sum: the reduce is defined by its order, not by it)
    # from 0.0: a lone -0.0 comes out as +0.0, as `s = 0.0; s += w` gives it
    assert bits(rank_ordered_sum(np.array([[-0.0]])))[0] == 0
    # NaN goes through, and is visible to a comparison of bit patterns only
    z = rank_ordered_sum(np.array([[1.0], [np.nan]]))
    assert np.isnan(z[0]) and not (z == z).any() and np.array_equal(bits(z), bits(z))


def test_finish_eval_restated_agrees_with_the_newton_driver(pkg, S):
    """One regularised iteration of pkg.newton_align on a synthetic (quadratic) evaluator: the result's score, transform
    probability and Hessian are finish_eval of the last raw evaluation -- ridge and f32 regularisation term, weighted by
    the n_pairs word -- bit for bit, and the first step runs along -H^-1 g of the finished first evaluation."""
    A = np.diag([40.0, 55.0, 70.0, 900.0, 1100.0, 1300.0]) + 3.0
    pstar = np.array([0.4, 0.05, 0.3, 0.002, -0.003, 0.25])
    n_pairs, n_total = 492977, 131072
    calls = []

    def ev(pose, T, need_h):
        d = pose - pstar
        w = pkg.pack_eval(8.0e4 - 0.5 * d @ A @ d, -A @ d, -A, nvtl_sum=3.5e4, n_with=1.2e5, n_pairs=n_pairs)
        calls.append((pose.copy(), w.copy(), need_h))
        return w

    reg_pose = S.pose_matrix(0.45, 0.02, 0.3, 0, 0, 0.26)
    guess = S.pose_matrix(0.1, -0.1, 0.2, 0, 0, 0.2)
    for ridge in (0, 1):
        del calls[:]
        prm = pkg.default_params(regularization_scale_factor=0.01, add_ridge=ridge, step_size=0.1, trans_epsilon=1e-4,
                                 max_iterations=1)
        r = pkg.newton_align(prm, n_total, guess, ev, regularization_pose=reg_pose)
        assert r["iterations"] >= 1 and len(calls) >= 2
        pose, w, need_h = calls[-1]
        assert need_h
        s, g, H = finish_eval_np(w, pose, True, add_ridge=bool(ridge), reg_pose=reg_pose, scale=0.01)
        assert bits(np.array([r["score"]]))[0] == bits(np.array([s]))[0], (r["score"], s)
        assert r["transform_probability"] == s / n_total
        assert np.array_equal(bits(r["hessian"]), bits(H))
        raw = finish_eval_np(w, pose, True)
        assert s != raw[0] and H[0, 0] != raw[2][0, 0] and (H[2, 2] != raw[2][2, 2]) == bool(ridge)
        # the weight is the n_pairs word: half the pairs, half the term (f32 rounding apart)
        w2 = w.copy()
        w2[30] = n_pairs // 2
        s2 = finish_eval_np(w2, pose, True, add_ridge=bool(ridge), reg_pose=reg_pose, scale=0.01)[0]
        assert (s2 - raw[0]) == pytest.approx((s - raw[0]) * (n_pairs // 2) / n_pairs, rel=1e-6)
        # the first Newton step: along -H^-1 g of the FINISHED first evaluation
        p0, w0, _ = calls[0]
        s0, g0, H0 = finish_eval_np(w0, p0, True, add_ridge=bool(ridge), reg_pose=reg_pose, scale=0.01)
        want = np.linalg.solve(H0, -g0)
        step = calls[1][0] - p0
        cos = abs(want @ step) / (np.linalg.norm(want) * np.linalg.norm(step))
        assert cos > 1 - 1e-12, cos
        unreg = np.linalg.solve(raw[2], -finish_eval_np(w0, p0, True)[1])
        assert abs(unreg @ step) / (np.linalg.norm(unreg) * np.linalg.norm(step)) < 1 - 1e-9
