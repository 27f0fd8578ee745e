"""ndt_align_batch against K serial ndt_align calls on C2 and C3: one process, clouds resident on the device, the same K
guesses (the config guess and perturbations of up to +-0.3 m / +-3 deg around it) both ways.  Wall clock around the
C-ABI calls, median of the reps; rounds per call = derivative launches of the batched call (ndt_timing.n_eval_launches).

    python tools/align_batch_probe.py [--reps 7] [--ks 1,2,4,8,16,32] [--configs c2,c3] [--out profiles/align_batch.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def guesses(S, cfg, K, seed=5):
    rng = np.random.default_rng(seed)
    out = [cfg["guess"]]
    while len(out) < K:
        x, y = rng.uniform(-0.3, 0.3, 2)
        yaw = np.deg2rad(rng.uniform(-3.0, 3.0))
        out.append(cfg["guess"] @ S.pose_matrix(x, y, 0.0, 0.0, 0.0, yaw))
    return np.ascontiguousarray(np.stack([np.asarray(G, np.float32).T.ravel() for G in out]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    S = pkg.synth
    L = pkg.lib()
    ks = [int(k) for k in a.ks.split(",")]
    lines = ["# tools/align_batch_probe.py --reps %d --ks %s --configs %s  (%s)" % (a.reps, a.ks, a.configs,
                                                                                  pkg.backend_info()[1]),
             "# config  K | batch ms/call  rounds/call  us/round | serial ms (K aligns)  evals (sum)  | batch/serial"]
    for name in a.configs.split(","):
        cfg = getattr(S, "config_" + name)()
        ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=cfg["resolution"], step_size=0.1,
                                               trans_epsilon=1e-4, max_iterations=35)
        ndt.setInputTarget(cfg["target"])
        ndt.setInputSource(cfg["source"])
        ndt.wait()
        for K in ks:
            g = guesses(S, cfg, K)
            gp = g.ctypes.data_as(C.POINTER(C.c_float))
            out = (pkg.Result * K)()
            one = pkg.Result()
            tb, ts, rounds, evals = [], [], 0, 0
            for r in range(a.reps + 2):   # (two warm-up reps)
                n0 = ndt.getTiming()["n_eval_launches"]
                t0 = time.perf_counter()
                rc = L.ndt_align_batch(ndt._h, gp, K, out)
                t1 = time.perf_counter()
                assert rc == 0, rc
                rounds = ndt.getTiming()["n_eval_launches"] - n0
                t2 = time.perf_counter()
                ev = 0
                for k in range(K):
                    assert L.ndt_align(ndt._h, g[k].ctypes.data_as(C.POINTER(C.c_float)), C.byref(one)) == 0
                    ev += one.n_evaluations
                t3 = time.perf_counter()
                evals = ev
                if r >= 2:
                    tb.append((t1 - t0) * 1e3)
                    ts.append((t3 - t2) * 1e3)
            mb, ms = float(np.median(tb)), float(np.median(ts))
            lines.append("%-7s %3d | %9.3f  %6d  %8.2f | %9.3f  %6d | %.3f" % (name.upper(), K, mb, rounds,
                                                                              mb / max(rounds, 1) * 1e3, ms, evals,
                                                                              mb / ms))
            print(lines[-1], flush=True)
        ndt.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines))


if __name__ == "__main__":
    main()
