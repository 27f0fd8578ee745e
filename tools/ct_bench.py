"""CALL LATENCY of one continuous-time evaluation beside one ordinary evaluation on the C2 source (not collected
by pytest).  What is timed is the call as a caller sees it, not the kernels: the two calls do not contain the same things
around their kernels (the CT call makes two launches, a device-to-host copy and a stream synchronise; the ordinary call
makes one launch and polls result slots in pinned memory), so the ratio below is a ratio of call latencies and says
nothing exact about evaluation cost on the device.  Kernel times want a kernel trace in a run of their own.

    python tools/ct_bench.py [--out FILE]

Scene: synth.config_c2 -- a 128 x 1024 scan (131 072 points) against the scan before it, 1.0 m leaf, DIRECT7.  The times
are the column's share of the revolution, as a spinning lidar gives them; the begin pose is the identity, the end pose the
scene's true offset (0.5 m, 2 degrees).  Reported, K = 1 with the Hessian, every call complete when it returns:
  - ndt_eval_derivatives_ct (k_ct_eval + the fixed-order sum + read-back);
  - ndt_eval_derivatives at the same pose on the same handle (this change does not touch it: it is the parent's);
  - their ratio.
Host clock around calls that end in a device synchronise, the two calls alternating in one loop, warmed up, median and
10 % / 90 % of the repetitions.  Writes what it prints to profiles/ct.txt (or --out)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def main():
    out = os.path.join(ROOT, "profiles", "ct.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    pkg = ge.load_package()
    synth = pkg.synth
    cfg = synth.config_c2()
    src = np.ascontiguousarray(cfg["source"], np.float32)
    n = len(src)
    az = np.arctan2(src[:, 1], src[:, 0])
    alpha = ((az + np.pi) / (2.0 * np.pi)).astype(np.float32)
    ndt = pkg.NormalDistributionsTransform(device_id=0, resolution=cfg["resolution"], step_size=0.1, trans_epsilon=1e-4,
                                           max_iterations=35)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(src)
    assert pkg.setSourceTimes(ndt, alpha) == n
    gt = np.asarray(cfg["gt"], np.float64)
    end = np.array([gt[0, 3], gt[1, 3], gt[2, 3], 0.0, 0.0, np.arctan2(gt[1, 0], gt[0, 0])])
    begin = np.zeros(6)
    gi = ndt.getGridInfo()
    e_ct = pkg.evalDerivativesCT(ndt, begin, end)[0]
    e_p2d = ndt.evalDerivatives(end)[0]
    say("Continuous-time NDT: one evaluation with one pose per point (DESIGN 7o) -- tools/ct_bench.py")
    say("%s: %d source points, %d leaves in %d cells, DIRECT7; end pose %.2f m, %.2f deg from the begin pose"
        % (cfg["name"], n, gi["n_leaves"], gi["n_cells"], np.linalg.norm(end[:3]), np.rad2deg(end[5])))
    say("pairs: %d (continuous time), %d (rigid at the end pose)" % (e_ct["n_pairs"], e_p2d["n_pairs"]))

    def ct():
        pkg.evalDerivativesCT(ndt, begin, end, raw=True)

    def p2d():
        ndt.evalDerivatives(end)

    for _ in range(20):
        ct()
        p2d()
    reps, ts = 300, {"ct": [], "p2d": []}
    for _ in range(reps):                                                   # alternating: both see the same box and moment
        for name, fn in (("ct", ct), ("p2d", p2d)):
            t = time.perf_counter()
            fn()
            ts[name].append(time.perf_counter() - t)
    med = {}
    for name, label in (("ct", "ndt_eval_derivatives_ct"), ("p2d", "ndt_eval_derivatives   ")):
        a = 1e6 * np.array(ts[name])
        med[name] = float(np.median(a))
        say("%s  K = 1, Hessian: call latency %8.1f us (10 %% %.1f, 90 %% %.1f; %d calls; host clock; launch, sum, read-back and wait included)"
            % (label, med[name], np.percentile(a, 10), np.percentile(a, 90), reps))
    say("ratio of call latencies (not of kernel times): %.2f" % (med["ct"] / med["p2d"]))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
