"""The asynchronous hand-off against the blocking one over the WHOLE handle API (the differential fuzz of
tests/test_gpu_handoff.py, whose vocabulary ends where the handle could set clouds, align, evaluate, read the grid, put
one keyframe and downsample): two engines, one blocking with every evaluation an ordinary launch, one asynchronous with
pre-launched kernels, both streams and the speculative first evaluation on, get the same calls; every observable --
return values as bytes, device outputs downloaded whole with their sentinel tail, refusals as ("error", code) -- must be
identical.  Host arrays handed to a call are overwritten (every byte 0xFF: NaN for floats) the moment it returns.

1. `Rig.call(engine, op, k)`: one operation and a small integer -> a comparable observation.
2. A producer -> consumer matrix: for every producer (a target or a source that the asynchronous engine leaves in
   flight) and every op of this file as the consumer, P then C with nothing in between, then one align.  Honest because
   (a) buildCounters()[1] + buildCounters()[2] (two-launch builds declined / gone through: steady-state builds only, the
   kind that stays pending) grows by one at every target producer whose cloud has a finite point.  The counters move when
   a build's verdict is COLLECTED: on the asynchronous engine the producer followed by wait() adds one (checked once per
   producer), and in every pair the blocking engine's sum has grown by one right after the producer while the
   asynchronous engine's has not moved yet -- its build is in flight when the consumer is called -- and both have grown
   alike after the pair.  The all-NaN target reaches neither counter (BG_NO_FINITE): its build was left pending if and
   only if the asynchronous call returned OK where the blocking one returned the error, which is asserted instead.
   (b) A failed deferred build survives every keep-grid consumer and is reported exactly once.
   Steady state at these sizes: every cloud of a few thousand points qualifies (bucket_build_fits: up to 1 310 720) as
   soon as the index grid and the leaf table hold it, so both engines are prepared by two builds of HULL, the 18 510
   points of all clouds, sources and keyframe scans together plus the corners of their box grown by 4 m (the largest
   cloud in points AND in cells: no later build outgrows the grid, BG_CAPACITY); confirmed on an MI355X with the clouds
   below (4 000-point two-plane pair, 16 x 256 lidar pair and subsamples).
3. Random sequences over the full vocabulary, three committed seeds (+ NDT_FUZZ_EXTRA_SEEDS); `sequence(seed)` is a pure
   function that needs no GPU, its coverage condition is checked by tests/test_api_sequences_cpu.py.
4. The transition table of the target itself, which two engines of the same code cannot see when both are wrong alike:
   every producer of a target, then every call that invalidates one, against a small Python restatement of the state
   (kind, cloud kept, reported points) -- after each step the statuses of grid, align, leaves and fitness and what the
   grid info reports are asserted, on both engines.  (csrc/ndt_target_state.* is that state; DESIGN.md has the table.)

Public methods of NormalDistributionsTransform that take the handle and are NOT in the vocabulary, and why
(tests/test_api_sequences_cpu.py checks that every public method is either called by the rig or named here):
close (ends the engine); computeTransformation (another name of align, the same function); setHandoffMode / getHandoffMode (the variable under test: fixed per engine); getHandoffTiming,
getTiming, enableKernelTiming, keepWarm / setKeepWarm (wall-clock figures, and kernel timing switches the pre-launched
kernels off); commInitRccl / commInitShm / commInitP2p / commInitHook / commP2pHandle / commRankCount / commP2pSelftest /
commP2pStats / commDestroy, setGlobalSourceSize (multi-rank jobs: tests/test_gpu_sharded.py); debugSortPairs, debugEvalLog,
debugEvalLogRead, prelaunchCounters, autoStreamPlacement, speculationCounters, setSpeculation, lostRowRetries,
prelaunchOverlapped, p2pHostFinishes, handoffCounters (debug seams that differ between the two engines by design;
buildCounters is read by the matrix); setNumThreads / getNumThreads, getResolution, getMinPointPerVoxel, getRecordFormat,
packetFormat, scanModelInfo, mapHasMoments, sourceSize, targetCount, keyframeCount, getFinalTransformation, hasConverged,
getFinalNumIteration, getNumEvaluations, getTransformationProbability, getNearestVoxelTransformationLikelihood,
getFitnessScore, getResult (host-side reads of what another op already returns; several are part of observations here);
scoreTransforms, calculateNearestVoxelTransformationLikelihood, proposePosesToSearch (thin variants of score /
calculateTransformationProbability / host-only); voxelDownsampleDevice (the host form, in the old vocabulary, runs it)."""
import os
import time

import numpy as np
import pytest

from test_deskew_cpu import make_trajectory
from test_gpu_deskew import download, f32_knots
from test_gpu_unproject import random_model
from test_packets_cpu import LEGACY, RNG19, encode, random_frame

pytestmark = pytest.mark.gpu

# ---- the vocabulary (no device needed from here to `sequence`) --------------------------------------------------------
OLD_OPS = ["target", "target_xyzi", "target_soa", "target_dev", "target_dev_deferred", "target_bad", "source", "source_soa",
           "source_dev", "source_view", "align", "eval", "score", "grid", "leaves", "step", "resolution", "search", "hessian",
           "maxit", "evalbatch", "keyframe", "downsample", "wait"]
NEW_OPS = [
    # consumers of target and source
    "fitness", "fitnessMany", "alignMany", "scorePoints", "scorePointsDevice", "filterSource", "filterSourceDevice",
    "transformSource", "getIterationHistory", "calculateTransformationProbability", "estimateXYCovarianceMultiNdt",
    "estimateXYCovarianceMultiNdtScore",
    # targets from elsewhere
    "addTarget", "createVoxelKdtree", "removeTarget", "setInputTargetFromKeyframes", "setInputTargetFromMap",
    "setInputTargetFromMapMoments",
    # keyframes
    "putKeyframe", "eraseKeyframe", "setInputSourceFromKeyframe", "putKeyframeDeskewed", "putKeyframeFromRanges",
    "putKeyframeFromPackets", "mapAddKeyframe", "mapCarveKeyframe",
    # voxel map
    "mapReset", "mapClear", "mapEnableMoments", "mapAdd", "mapAddDevice", "mapInfo", "mapExport", "mapExportDevice",
    "mapExportMoments", "mapCrop", "mapExportState", "mapExportStateDevice", "mapImportState", "mapImportStateDevice",
    "mapCarve", "mapCarveDevice",
    # scan side
    "deskew", "deskewDevice", "setScanModel", "clearScanModel", "unproject", "unprojectDevice", "setPacketFormat",
    "beginPacketFrame", "pushPackets", "unprojectPacketFrame", "unprojectPacketFrameDevice", "decodePacketFrameDevice",
    "packetFrameInfo",
    # setters that invalidate state
    "setRecordFormat", "setRegularizationPose", "unsetRegularizationPose", "sourceChanged", "setTransformationEpsilon",
    "setOutlierRatio", "setMinPointPerVoxel"]
OPS = OLD_OPS + NEW_OPS
# the producers of the matrix: (op, k) -- what the asynchronous engine leaves in flight
PRODUCERS = {"target_host": ("target", 1), "target_xyzi": ("target_xyzi", 2), "target_dev_deferred": ("target_dev_deferred", 3),
             "source_host": ("source", 1), "putKeyframe": ("putKeyframe", 4), "target_from_keyframes": ("setInputTargetFromKeyframes", 1),
             "target_bad": ("target_bad", 0)}
PRODUCER_OPS = sorted({op for op, _ in PRODUCERS.values()})
TARGET_PRODUCERS = ("target_host", "target_xyzi", "target_dev_deferred", "target_from_keyframes")
# calls that need the grid / that leave it alone (the deferred-failure test)
GRID_CONSUMERS = [("fitness", 0), ("scorePoints", 0), ("filterSource", 1), ("alignMany", 0), ("align", 0)]
KEEP_GRID_CONSUMERS = [("mapAdd", 0), ("mapAddDevice", 1), ("mapAddKeyframe", 0), ("mapExport", 0), ("mapExportDevice", 0),
                       ("mapExportMoments", 0), ("mapCrop", 0), ("mapExportState", 0), ("mapExportStateDevice", 1),
                       ("mapImportState", 1), ("mapImportStateDevice", 1), ("mapCarve", 0), ("mapCarveDevice", 0),
                       ("mapCarveKeyframe", 0), ("downsample", 0), ("deskew", 1), ("deskewDevice", 1), ("unproject", 1),
                       ("unprojectDevice", 2), ("pushPackets", 0), ("unprojectPacketFrame", 2), ("unprojectPacketFrameDevice", 1),
                       ("decodePacketFrameDevice", 0), ("putKeyframeFromPackets", 0), ("putKeyframeFromRanges", 1),
                       ("putKeyframeDeskewed", 1), ("putKeyframe", 2), ("packetFrameInfo", 0), ("mapInfo", 0)]

# Weights: what builds state up (targets, sources, keyframes, the map, the packet frame) is drawn more often than what
# tears it down (a failing target, clearing the map or the scan model, erasing), so that most calls meet an engine that can
# serve them; a refusal is an observation like any other, but a sequence of refusals tests little.
WEIGHT = {"target": 4, "target_xyzi": 4, "target_dev_deferred": 4, "source": 4, "putKeyframe": 4, "setInputTargetFromKeyframes": 4,
          "target_bad": 2.5, "align": 6, "target_soa": 2, "target_dev": 2, "source_soa": 2, "eval": 2, "mapAdd": 3, "mapReset": 3,
          "setPacketFormat": 3, "beginPacketFrame": 2, "pushPackets": 4, "setInputSourceFromKeyframe": 2, "addTarget": 2,
          "setScanModel": 1.2, "mapClear": 0.8, "clearScanModel": 0.8, "eraseKeyframe": 1, "removeTarget": 1, "wait": 1}
WEIGHTS = np.array([float(WEIGHT.get(op, 1.5)) for op in OPS])
WEIGHTS /= WEIGHTS.sum()
LENGTH = 800
K_RANGE = 24
# The first three seeds that meet the coverage condition of tests/test_api_sequences_cpu.py at this length (the test
# prints, per seed, how many calls were served and which ops never were: about three calls in four, and over the three
# seeds together every op but the failing target).
SEEDS = [1, 4, 7]


def sequence(seed, length=LENGTH):
    """seed -> [(op, k)]: a pure function of its arguments (no device, no global state)"""
    rng = np.random.default_rng(seed)
    idx = rng.choice(len(OPS), size=length, p=WEIGHTS)
    ks = rng.integers(0, K_RANGE, size=length)
    return [(OPS[int(i)], int(k)) for i, k in zip(idx, ks)]


def extra_seeds():
    return list(range(100, 100 + int(os.environ.get("NDT_FUZZ_EXTRA_SEEDS", "0"))))


# ---- observations -----------------------------------------------------------------------------------------------------
def obs(x):
    """anything a call returns -> something == compares bit for bit (a NaN equals itself)"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (float, np.floating)):
        return np.float64(x).tobytes()
    if isinstance(x, (bool, int, np.integer, str, bytes)) or x is None:
        return x if not isinstance(x, np.integer) else int(x)
    if isinstance(x, dict):
        return tuple((k, obs(x[k])) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return tuple(obs(v) for v in x)
    raise TypeError(type(x))


RESULT_FIELDS = ("T", "pose", "converged", "iterations", "n_evaluations", "hessian", "score", "transform_probability", "nvtl",
                 "n_pairs", "n_points_with_neighbors")


def result_obs(r):
    return obs({k: r[k] for k in RESULT_FIELDS})


def consumed(*arrays):
    """the caller's memory after the call: every byte 0xFF (a float NaN, an integer -1)"""
    for a in arrays:
        if a is not None:
            a.view(np.uint8).reshape(-1)[:] = 0xFF


def xyzi(a, fill=3.5):
    out = np.full((len(a), 8), fill, np.float32)
    out[:, :3] = a
    return out


def refused(r):
    """an observation that is a refusal (of the call itself, or of the device form whose outputs are still downloaded)"""
    return isinstance(r, tuple) and len(r) > 0 and (r[0] == "error" or refused(r[0]))


def brief(r):
    return r if not isinstance(r, tuple) or (len(r) == 2 and r[0] == "error") else "..."


# ---- the rig: data, device buffers, the two engines -------------------------------------------------------------------
N_COLS, N_ROWS, CPP = 24, 5, 4           # the scan model and packet frame of tests/test_gpu_packets.py
BUF, TAIL = 16384, 16                    # elements of a device output buffer (8 bytes each) and its sentinel tail
KF_IDS = (3, 7, 9)
MAP_LEAVES = (1.0, 1.5)                  # (the resolutions of the old vocabulary: a map's moments become a target only at its leaf)
SENTINEL = 0xA5
STATE_CAP, STATE_WIDTHS = 2048, (12, 4, 16, 72)   # records an exported map state may hold on the device, bytes of each array's record


class Rig:
    def __init__(self, pkg, S, hipmem):
        self.pkg, self.S, self.hip = pkg, S, hipmem
        a, b = S.config_c1(max_points=4000), S.config_c2(beams=16, cols=256)
        self.clouds = [a["target"], b["target"][::2], a["target"][::3] + np.float32(0.25), b["target"]]
        self.sources = [a["source"], b["source"][::4], a["source"][::2]]
        self.guesses = [a["guess"], b["guess"], a["guess"]]
        self.bad = np.full((3000, 3), np.nan, np.float32)
        self.kf_clouds = [self.sources[0][::2], self.sources[1], self.sources[2][::3], np.zeros((0, 3), np.float32)]
        self.poses = [S.pose_matrix(0.3 * j, -0.2 * j, 0.05 * j, 0.0, 0.0, 0.02 * j) for j in range(4)]
        # the small clouds the map is made of (a few hundred voxels at either leaf): the two-plane pair within 6 m
        near = lambda c: np.ascontiguousarray(c[(np.abs(c[:, :2] - np.median(c[:, :2], 0)) < 6.0).all(1)])   # noqa: E731
        self.map_clouds = [near(a["target"]), near(a["source"]), near(a["target"][::2] + np.float32(0.4))]
        self.tiles = [near(a["target"]), near(a["target"] + np.float32([4.0, 0.0, 0.0])), near(a["target"] + np.float32([0.0, 5.0, 0.5]))]
        every = self.clouds + self.sources + [S.transform(T, c) for T in self.poses for c in self.kf_clouds if len(c)]
        pts = np.concatenate(self.clouds + self.sources)
        lo, hi = np.min([c.min(0) for c in every], 0) - 4.0, np.max([c.max(0) for c in every], 0) + 4.0
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float32)
        self.hull = np.ascontiguousarray(np.concatenate([pts, corners]), np.float32)
        up3 = lambda c: [hipmem.upload(np.ascontiguousarray(c[:, ax])) for ax in range(3)]   # noqa: E731
        self.dev = [up3(c) for c in self.clouds]
        self.dsrc = [up3(c) for c in self.sources]
        self.dmap = [up3(c) for c in self.map_clouds]
        self.dmap_i = [hipmem.upload(np.linspace(0.0, 200.0, len(c)).astype(np.float32)) for c in self.map_clouds]
        self.view = up3(self.sources[0])                      # a viewed source the caller rewrites in place
        self.view_n = min(len(s) for s in self.sources)
        # deskew: one time per point and two trajectories
        self.traj = []
        for n_knots, seed in ((2, 71), (5, 72)):
            kt, kp = make_trajectory(n_knots, seed)
            self.traj.append((f32_knots(kt), kp))
        self.times = [np.linspace(-0.05, 0.45, len(s)).astype(np.float32) for s in self.sources]
        self.dtimes = [hipmem.upload(t) for t in self.times]
        self.dinten = [hipmem.upload(np.linspace(0.0, 250.0, len(s)).astype(np.float32)) for s in self.sources]
        self.box = pkg.ScanFilter.from_vehicle_box([0.0, 0.0, 0.0], [6.0, 6.0, 6.0], z_band=(-30.0, 30.0), intensity_keep_min=100.0)
        # the scan side: two models, a range image within 40 m (a keyframe made of it stays inside the index grid's reach)
        self.models = [random_model(N_COLS, N_ROWS, 7), random_model(N_COLS, N_ROWS, 8)]
        self.frames, self.packets = {}, {}
        for profile in (RNG19, LEGACY):
            f = random_frame(profile, N_COLS, N_ROWS, 31 + profile, dt_ns=int(0.4e9 / N_COLS))
            f["range_mm"] = (f["range_mm"] % np.uint32(40000)).astype(np.uint32)
            self.frames[profile] = f
            self.packets[profile] = [encode(S, profile, N_COLS, N_ROWS, CPP, f, frame_id=7 + j, seed=2 + j) for j in range(2)]
        img = self.frames[RNG19]
        self.col_t = np.linspace(0.0, 0.4, N_COLS).astype(np.float32)
        self.d_range = hipmem.upload(img["range_mm"].ravel())
        self.d_refl = hipmem.upload(img["reflectivity"].ravel())
        self.d_col_t = hipmem.upload(self.col_t)
        self.gate = pkg.RangeGate(0.5, 35.0, row_step=2)
        # output buffers, shared by both engines (every call with a device output returns with its launches complete)
        self.fill = np.full((BUF + TAIL) * 8, SENTINEL, np.uint8)
        self.out = [hipmem.upload(self.fill) for _ in range(8)]
        self.messages = {}                                    # per engine: the text of its last refusal
        self._lent = []                                       # copies of shared host arrays lent to the op in progress (lend)

    # -- engines --
    def engine(self, mode):
        pkg = self.pkg
        e = pkg.NormalDistributionsTransform(device_id=0, resolution=1.0, step_size=0.1, trans_epsilon=1e-4, max_iterations=35,
                                             prelaunch=pkg.PRELAUNCH_OFF if mode == pkg.HANDOFF_SYNC else pkg.PRELAUNCH_AUTO)
        e.setHandoffMode(mode)
        e.tag = "blocking" if mode == pkg.HANDOFF_SYNC else "asynchronous"
        # each engine exports its map state into device arrays of its own (it re-imports them later)
        # (ijk 12, count 4, sums 16 and moments 72 bytes a record; never refilled: both engines' arrays have one history)
        e.dstate = [self.hip.upload(np.full(STATE_CAP * w + 8 * TAIL, SENTINEL, np.uint8)) for w in STATE_WIDTHS]
        e.dstate_n = None
        e.saved = None
        return e

    def prepare(self, e):
        """The state every pair of the matrix starts from: a steady-state grid (the next build is the optimistic kind), a
        source, a small map with moments, a scan model, two keyframes, a packet frame begun and pushed."""
        pkg = self.pkg
        e.setParams(resolution=1.0, step_size=0.1, max_iterations=35, search_method=pkg.DIRECT7, hessian_mode=pkg.HESSIAN_FULL,
                    trans_epsilon=1e-4, outlier_ratio=0.55, min_points_per_voxel=6,
                    regularization_scale_factor=pkg.default_params().regularization_scale_factor)
        e.setRecordFormat(pkg.RECORDS_F64)
        e.unsetRegularizationPose()
        for erase, ids in ((e.eraseKeyframe, KF_IDS), (e.removeTarget, (11, 12, 13))):
            for id_ in ids:
                try:
                    erase(id_)
                except pkg.NdtError:
                    pass
        e.addTarget(self.tiles[0], 11)                        # (two overlapping tiles of a multi-grid target, not assembled)
        e.addTarget(self.tiles[1], 12)
        e.setInputTarget(self.hull)
        e.wait()
        e.setInputSource(self.sources[0])
        e.putKeyframe(KF_IDS[0], self.kf_clouds[0])
        e.putKeyframe(KF_IDS[1], self.kf_clouds[1])
        e.mapReset(1.0, with_intensity=False, initial_capacity=64)
        e.mapEnableMoments()
        e.mapAdd(self.map_clouds[0])
        e.setScanModel(*self.models[0])
        e.setPacketFormat(RNG19, CPP)
        e.beginPacketFrame()
        e.pushPackets(self.packets[RNG19][0])
        e.saved = e.mapExportState()
        self.call(e, "mapExportStateDevice", 0)
        e.align(self.guesses[0])
        e.wait()

    # -- device outputs --
    def fresh(self, *slots):
        """output buffers, every byte the sentinel (grab() refills them: no copy stands between two calls of an engine)"""
        return [self.out[j] for j in slots]

    def grab(self, *slots):
        """the whole buffers, sentinel tails included (and the tails intact: nothing may be written behind BUF elements)"""
        res = []
        for j in slots:
            raw = download(self.hip, self.out[j], (BUF + TAIL) * 8, np.uint8)
            assert np.all(raw[BUF * 8:] == SENTINEL), "a device output was written behind its capacity"
            res.append(raw.tobytes())
            self.hip.write(self.out[j], self.fill)
        return tuple(res)

    # -- one operation --
    def lend(self, a):
        """a copy of a shared host array (a transform, a pose, knot times or poses) for ONE call: call() overwrites it when
        the op returns, as the ops themselves do with their clouds"""
        c = np.array(a, copy=True, order="C")
        self._lent.append(c)
        return c

    def pose(self, j):
        return self.lend(self.poses[j])

    def knots(self, j):
        return self.lend(self.traj[j][0]), self.lend(self.traj[j][1])

    def call(self, e, op, k):
        """One operation -> a comparable observation, ("error", code) for a refusal."""
        mark = len(self._lent)
        try:
            return self._call(e, op, k)
        except self.pkg.NdtError as err:
            self.messages[e.tag] = str(err)
            return ("error", err.code)
        finally:
            consumed(*self._lent[mark:])
            del self._lent[mark:]

    def _call(self, e, op, k):   # noqa: C901
        pkg, hip = self.pkg, self.hip
        clouds, sources, guesses = self.clouds, self.sources, self.guesses
        T = self.lend(guesses[k % 3])
        # ---- the old vocabulary (tests/test_gpu_handoff.py), the host arrays consumed ----
        if op == "target":
            t = clouds[k % 4].copy(); e.setInputTarget(t); consumed(t); return "ok"
        if op == "target_xyzi":
            t = xyzi(clouds[k % 4]); e.setInputTarget(t); consumed(t); return "ok"
        if op == "target_soa":
            t = [np.ascontiguousarray(clouds[k % 4][:, ax]) for ax in range(3)]; e.setInputTargetSoA(*t); consumed(*t); return "ok"
        if op == "target_dev":
            d = self.dev[k % 4]; e.setInputTargetDevice(d[0], d[1], d[2], len(clouds[k % 4])); return "ok"
        if op == "target_dev_deferred":
            d = self.dev[k % 4]; e.setInputTargetDeviceDeferred(d[0], d[1], d[2], len(clouds[k % 4])); return "ok"
        if op == "target_bad":
            t = self.bad.copy(); e.setInputTarget(t); return "ok"
        if op == "source":
            s = sources[k % 3].copy(); e.setInputSource(s); consumed(s); return "ok"
        if op == "source_soa":
            s = [np.ascontiguousarray(sources[k % 3][:, ax]) for ax in range(3)]; e.setInputSourceSoA(*s); consumed(*s); return "ok"
        if op == "source_dev":
            d = self.dsrc[k % 3]; e.setInputSourceDevice(d[0], d[1], d[2], len(sources[k % 3])); return "ok"
        if op == "source_view":
            d = self.dsrc[k % 3]; e.setInputSourceDeviceView(d[0], d[1], d[2], len(sources[k % 3])); return "ok"
        if op == "align":
            e.align(T); return result_obs(e.getResult())
        if op == "eval":
            ev = e.evalDerivatives(self.lend([0.3, 0.05, 0.0, 0.0, 0.01, 0.02 * (k % 5)]))[0]
            return obs((ev["score"], ev["n_pairs"], ev["gradient"], ev["hessian"]))
        if op == "score":
            return obs(e.scoreTransform(T))
        if op == "grid":
            g = e.getGridInfo(); return obs({f: g[f] for f in g if f != "ms_build"})
        if op == "leaves":
            return obs(e.getLeaves())
        if op == "step":
            e.setStepSize(0.1 if k % 2 else 0.05); return "ok"
        if op == "resolution":
            e.setResolution(1.0 if k % 2 else 1.5); return "ok"
        if op == "search":
            e.setNeighborhoodSearchMethod((pkg.DIRECT7, pkg.DIRECT1, pkg.KDTREE, pkg.DIRECT26)[k % 4]); return "ok"
        if op == "hessian":
            e.setParams(hessian_mode=pkg.HESSIAN_GAUSS_NEWTON if k % 2 else pkg.HESSIAN_FULL); return "ok"
        if op == "maxit":
            e.setMaximumIterations((35, 2, 0, 12)[k % 4]); return "ok"
        if op == "evalbatch":
            P = self.lend([[0.3, 0.05, 0.0, 0.0, 0.01, 0.02 * j] for j in range(1 + k % 5)])
            return obs([(ev["score"], ev["n_pairs"], ev["hessian"]) for ev in e.evalDerivatives(P)])
        if op == "keyframe":
            s = sources[k % 3].copy(); e.putKeyframe(7, s); consumed(s); e.setInputSourceFromKeyframe(7); return e.sourceSize()
        if op == "downsample":
            c = clouds[k % 4][::5].copy(); out = e.voxelDownsample(c, 0.75); consumed(c); return obs(out)
        if op == "wait":
            e.wait(); return "ok"

        # ---- consumers of target and source ----
        if op == "fitness":
            kw = ({}, dict(max_range=4.0), dict(max_range=1.0, per_point=True))[k % 3]
            return obs(e.fitness(T, **kw))
        if op == "fitnessMany":
            return obs(e.fitnessMany([self.lend(g) for g in guesses[:1 + k % 3]], **({} if k % 2 else dict(max_range=4.0))))
        if op == "alignMany":
            K = (1, 3, 6)[k % 3]
            gs = [self.lend(guesses[j % 3] @ self.S.pose_matrix(0.05 * j, 0.0, 0.0, 0.0, 0.0, 0.01 * j)) for j in range(K)]
            return tuple(result_obs(r) for _, r in e.alignMany(gs))
        if op == "scorePoints":
            return obs(e.scorePoints(T, fields=None if k % 2 else ("nearest_voxel_score", "best_voxel")))
        if op == "scorePointsDevice":
            o = self.fresh(0, 1, 2, 3)
            e.scorePointsDevice(T, o[0], o[1] if k % 2 else None, o[2], o[3], BUF)
            return self.grab(0, 1, 2, 3)
        if op == "filterSource":
            return obs(e.filterSource(T, (0.0, 0.5, 0.05)[k % 3], keep_below=bool(k // 3 % 2)))
        if op == "filterSourceDevice":
            o = self.fresh(0, 1, 2, 3)
            cap = 7 if k % 4 == 3 else BUF                    # (7: below any selection of min_score 0)
            thr, below = ((0.0, False) if k % 4 == 3 else ((0.0, 0.5, 0.05)[k % 3], bool(k // 4 % 2)))
            try:
                m = e.filterSourceDevice(T, thr, below, o[0], o[1], o[2], o[3] if k % 2 else None, cap)
            except pkg.NdtError as err:
                m = ("error", err.code, e.last_filter_count)
            return (m,) + self.grab(0, 1, 2, 3)
        if op == "transformSource":
            return obs(e.transformSource(T))
        if op == "getIterationHistory":
            return obs(e.getIterationHistory())
        if op == "calculateTransformationProbability":
            s = sources[k % 3].copy(); r = e.calculateTransformationProbability(s, T); consumed(s); return obs(r)
        if op in ("estimateXYCovarianceMultiNdt", "estimateXYCovarianceMultiNdtScore"):
            e.align(T)
            r = e.getResult()
            poses = [self.lend(p) for p in e.proposePosesToSearch([0.0, 0.3, -0.3, 0.0], [0.3, 0.0, 0.0, -0.3])]
            if op == "estimateXYCovarianceMultiNdt":
                return (result_obs(r), obs(e.estimateXYCovarianceMultiNdt(poses)))
            return (result_obs(r), obs(e.estimateXYCovarianceMultiNdtScore(poses, 0.1 + 0.05 * (k % 3))))

        # ---- targets from elsewhere ----
        if op == "addTarget":
            c = self.tiles[k % 3].copy(); e.addTarget(c, 11 + k % 3); consumed(c); return e.targetCount()
        if op == "createVoxelKdtree":
            e.createVoxelKdtree(); g = e.getGridInfo(); return obs({f: g[f] for f in g if f != "ms_build"})
        if op == "removeTarget":
            e.removeTarget(11 + k % 3); return e.targetCount()
        if op == "setInputTargetFromKeyframes":
            ids = ([KF_IDS[0]], [KF_IDS[0], KF_IDS[1]], list(KF_IDS), [KF_IDS[2]], [KF_IDS[1], KF_IDS[1]], [KF_IDS[2], KF_IDS[0]])[k % 6]
            e.setInputTargetFromKeyframes(ids, [self.pose((j + k) % 4) for j in range(len(ids))]); return "ok"
        if op == "setInputTargetFromMap":
            e.setInputTargetFromMap(min_points=1 + k % 3); return "ok"
        if op == "setInputTargetFromMapMoments":
            if k % 2:
                e.setInputTargetFromMapMoments()
            else:
                e.setInputTargetFromMapMoments([-3.0, -5.0, -4.0], [4.0, 5.5, 6.0])
            return "ok"

        # ---- keyframes ----
        if op == "putKeyframe":
            c = self.kf_clouds[k % 4].copy(); e.putKeyframe(KF_IDS[k // 4 % 3], c); consumed(c); return e.keyframeCount()
        if op == "eraseKeyframe":
            e.eraseKeyframe(KF_IDS[k % 3]); return (e.keyframeCount(), e.sourceSize())
        if op == "setInputSourceFromKeyframe":
            e.setInputSourceFromKeyframe(KF_IDS[k % 3]); return e.sourceSize()
        if op == "putKeyframeDeskewed":
            j = k % 3
            c = np.concatenate([sources[j], np.linspace(0.0, 250.0, len(sources[j]), dtype=np.float32)[:, None]], 1)
            t = self.times[j].copy()
            kt, kp = self.knots(k % 2)
            m = e.putKeyframeDeskewed(KF_IDS[k // 3 % 3], c, t, kt, kp, filter=self.box if k % 2 else None,
                                      intensity_column=3 if k % 2 else None)
            consumed(c, t)
            return (m, e.keyframeCount())
        if op == "putKeyframeFromRanges":
            img = self.frames[RNG19]
            r, refl, ct = img["range_mm"].copy(), img["reflectivity"].copy(), self.col_t.copy()
            kt, kp = self.knots(k % 2) if k % 3 else (None, None)
            m = e.putKeyframeFromRanges(KF_IDS[k % 3], r, refl if k % 2 else None, ct, knot_t=kt, knot_poses=kp,
                                        gate=self.gate if k % 2 else None)
            consumed(r, refl, ct)
            return (m, e.keyframeCount())
        if op == "putKeyframeFromPackets":
            kt, kp = self.knots(k % 2) if k % 3 else (None, None)
            r = e.putKeyframeFromPackets(KF_IDS[k % 3], knot_t=kt, knot_poses=kp, gate=self.gate if k % 2 else None,
                                         with_signal=bool(k % 2), with_nir=bool(k % 4 == 1))
            return (obs(r), e.keyframeCount())
        if op == "mapAddKeyframe":
            e.mapAddKeyframe(KF_IDS[k % 3], self.pose(k % 4)); return obs(e.mapInfo())
        if op == "mapCarveKeyframe":
            return obs(e.mapCarveKeyframe(KF_IDS[k % 3], [0.0, 0.0, 3.0], self.pose(k % 4), min_misses=1 + k % 2, dry_run=bool(k % 4 == 3)))

        # ---- the voxel map ----
        if op == "mapReset":
            e.mapReset(MAP_LEAVES[k % 2], with_intensity=bool(k // 2 % 4 == 3), initial_capacity=64)
            if k % 4 != 3:                                    # (most maps keep moments; the others leave mapEnableMoments something to do)
                e.mapEnableMoments()
            return (e.mapHasMoments(), obs(e.mapInfo()))
        if op == "mapClear":
            e.mapClear()
            return ("cleared", self.call(e, "mapInfo", 0))    # (the refusal: no map)
        if op == "mapEnableMoments":
            if k % 2:                                         # on a fresh map without moments (the only state that accepts the call)
                e.mapReset(MAP_LEAVES[k // 2 % 2], with_intensity=False, initial_capacity=64)
            e.mapEnableMoments(); return e.mapHasMoments()
        if op == "mapAdd":
            j = k % 3
            c = self.map_clouds[j].copy()
            if k // 3 % 2:                                    # with an intensity column (a map that keeps none ignores it)
                c = np.ascontiguousarray(np.concatenate([c, np.linspace(0.0, 200.0, len(c), dtype=np.float32)[:, None]], 1))
                e.mapAdd(c, intensity_column=3, pose=self.pose(k % 4) if k % 2 else None)
            else:
                e.mapAdd(c, pose=self.pose(k % 4) if k % 2 else None)
            consumed(c)
            return obs(e.mapInfo())
        if op == "mapAddDevice":
            j = k % 3
            d = self.dmap[j]
            e.mapAddDevice(d[0], d[1], d[2], len(self.map_clouds[j]), d_intensity=self.dmap_i[j] if k // 3 % 2 else None,
                           pose=self.pose(k % 4) if k % 2 else None)
            return obs(e.mapInfo())
        if op == "mapInfo":
            return obs(e.mapInfo())
        if op == "mapExport":
            if k % 2:
                return obs(e.mapExport(min_points=1 + k % 3, columns=5, intensity_column=4, with_counts=True))
            return obs(e.mapExport(min_points=1 + k % 3))
        if op == "mapExportDevice":
            o = self.fresh(0, 1, 2, 3, 4)
            m = e.mapExportDevice(o[0], o[1], o[2], BUF, min_points=1 + k % 3, o_intensity=o[3] if k % 2 else None, o_count=o[4])
            return (m,) + self.grab(0, 1, 2, 3, 4)
        if op == "mapExportMoments":
            return obs(e.mapExportMoments(min_points=1 + k % 3))
        if op == "mapCrop":
            n = e.mapCrop([-3.0, -5.0, -40.0], [4.0, 5.5, 60.0], remove_inside=bool(k % 2))
            return (n, obs(e.mapInfo()))
        if op == "mapExportState":
            st = e.mapExportState(*(([-6.0, -2.0, -40.0], [6.0, 9.0, 60.0]) if k % 2 else (None, None)))
            e.saved = st
            return obs(st)
        if op == "mapExportStateDevice":
            box = ([-6.0, -2.0, -40.0], [6.0, 9.0, 60.0]) if k % 2 else (None, None)
            e.dstate_n = None                                 # (a refused export leaves nothing to import)
            mom = e.mapHasMoments()
            m = e.mapExportStateDevice(e.dstate[0], e.dstate[1], e.dstate[2], e.dstate[3] if mom else None, STATE_CAP, *box)
            e.dstate_n = (m, e.mapInfo()["leaf"], mom)
            raw = [download(hip, p, STATE_CAP * w + 8 * TAIL, np.uint8) for p, w in zip(e.dstate, STATE_WIDTHS)]
            assert all(np.all(r[STATE_CAP * w:] == SENTINEL) for r, w in zip(raw, STATE_WIDTHS)), "an export wrote behind its capacity"
            return (m,) + tuple(r.tobytes() for r in raw)
        if op == "mapImportState":
            st = e.saved
            if st is None:
                return "nothing exported yet"
            arrays = [None if st[f] is None else st[f].copy() for f in ("ijk", "count", "sums", "moments")]
            e.mapImportState(leaf=st["leaf"], ijk=arrays[0], count=arrays[1], sums=arrays[2], moments=arrays[3] if k % 4 else None)
            consumed(*arrays)
            return obs(e.mapInfo())
        if op == "mapImportStateDevice":
            if e.dstate_n is None:
                return "nothing exported yet"
            m, leaf, mom = e.dstate_n
            e.mapImportStateDevice(leaf, e.dstate[0], e.dstate[1], e.dstate[2], e.dstate[3] if mom else None, m)
            return obs(e.mapInfo())
        if op == "mapCarve":
            c = self.map_clouds[k % 3].copy()
            r = e.mapCarve(c, [0.5, -0.5, 4.0], pose=self.pose(k % 4) if k % 2 else None, min_misses=1 + k % 2, keep_last=k % 3,
                           dry_run=bool(k % 4 == 3))
            consumed(c)
            return (obs(r), self.call(e, "mapInfo", 0))
        if op == "mapCarveDevice":
            j = k % 3
            d = self.dmap[j]
            r = e.mapCarveDevice(d[0], d[1], d[2], len(self.map_clouds[j]), [0.5, -0.5, 4.0], pose=self.pose(k % 4) if k % 2 else None,
                                 min_misses=1 + k % 2, dry_run=bool(k % 4 == 3))
            return (obs(r), self.call(e, "mapInfo", 0))

        # ---- the scan side ----
        if op == "deskew":
            j = k % 3
            c = np.ascontiguousarray(np.concatenate([sources[j], np.linspace(0.0, 250.0, len(sources[j]), dtype=np.float32)[:, None]], 1))
            t = self.times[j].copy()
            kt, kp = self.knots(k // 2 % 2)
            r = e.deskew(c, t, kt, kp, filter=self.box if k % 2 else None, intensity_column=3, with_index=True)   # aligned / compacting
            consumed(c, t)
            return obs(r)
        if op == "deskewDevice":
            j = k % 3
            d, n = self.dsrc[j], len(sources[j])
            o = self.fresh(0, 1, 2, 3, 4)
            kt, kp = self.knots(k // 2 % 2)
            m = e.deskewDevice(d[0], d[1], d[2], self.dtimes[j], n, kt, kp, o[0], o[1], o[2], BUF, filter=self.box if k % 2 else None,
                               d_intensity=self.dinten[j], o_intensity=o[3], d_index=o[4])
            return (m,) + self.grab(0, 1, 2, 3, 4)
        if op == "setScanModel":
            m = [a.copy() for a in self.models[k % 2]]; e.setScanModel(*m); consumed(*m); return (e.scanModelInfo(), e.packetFormat())
        if op == "clearScanModel":
            e.clearScanModel(); return (e.scanModelInfo(), e.packetFormat())
        if op == "unproject":
            img = self.frames[RNG19]
            r, refl, ct = img["range_mm"].copy(), img["reflectivity"].copy(), self.col_t.copy()
            kt, kp = self.knots(k % 2) if k % 3 else (None, None)
            res = e.unproject(r, refl, ct, knot_t=kt, knot_poses=kp, gate=self.gate if k % 2 else None,
                              filter=self.box if k // 2 % 2 else None, with_t=True, with_index=True)
            consumed(r, refl, ct)
            return obs(res)
        if op == "unprojectDevice":
            o = self.fresh(0, 1, 2, 3, 4, 5)
            kt, kp = self.knots(k % 2) if k % 3 else (None, None)
            try:
                m = e.unprojectDevice(self.d_range, self.d_refl, self.d_col_t, o[0], o[1], o[2], BUF, knot_t=kt, knot_poses=kp,
                                      gate=self.gate if k % 2 else None, filter=self.box if k // 2 % 2 else None, o_intensity=o[3],
                                      o_t=o[4], d_index=o[5])
            except pkg.NdtError as err:
                m = ("error", err.code, e.last_unproject_count)
            return (m,) + self.grab(0, 1, 2, 3, 4, 5)
        if op == "setPacketFormat":
            e.setPacketFormat((RNG19, LEGACY)[k % 2], CPP); return e.packetFormat()
        if op == "beginPacketFrame":
            e.beginPacketFrame(); return obs(e.packetFrameInfo())
        if op == "pushPackets":
            profile = e.packetFormat()[0]
            p = self.packets[profile if profile in (RNG19, LEGACY) else RNG19][k // 3 % 2].copy()
            if k % 3 == 0:                                    # in one piece
                taken = [e.pushPackets(p)]
            else:                                             # in pieces (k % 3 == 2: the second half first)
                halves = [p[:len(p) // 2].copy(), p[len(p) // 2:].copy()][::-1 if k % 3 == 2 else 1]
                taken = [e.pushPackets(h) for h in halves]
                consumed(*halves)
            consumed(p)
            return (tuple(taken), obs(e.packetFrameInfo()))
        if op == "unprojectPacketFrame":
            kt, kp = self.knots(k % 2) if k % 3 else (None, None)
            return obs(e.unprojectPacketFrame(knot_t=kt, knot_poses=kp, gate=self.gate if k % 2 else None,
                                              filter=self.box if k // 2 % 2 else None, with_t=True, with_index=True,
                                              with_signal=bool(k % 2), with_nir=bool(k % 4 < 2)))
        if op == "unprojectPacketFrameDevice":
            o = self.fresh(0, 1, 2, 3, 4, 5, 6, 7)
            kt, kp = self.knots(k % 2) if k % 3 else (None, None)
            try:
                m = e.unprojectPacketFrameDevice(o[0], o[1], o[2], BUF, knot_t=kt, knot_poses=kp, gate=self.gate if k % 2 else None,
                                                 filter=self.box if k // 2 % 2 else None, o_intensity=o[3], o_t=o[4],
                                                 d_index=o[5] if k % 4 else None, d_signal=o[6], d_nir=o[7] if k % 2 else None)
            except pkg.NdtError as err:
                m = ("error", err.code, e.last_unproject_count)
            return (m,) + self.grab(0, 1, 2, 3, 4, 5, 6, 7)
        if op == "decodePacketFrameDevice":
            o = self.fresh(0, 1, 2, 3, 4)
            e.decodePacketFrameDevice(o[0], o[1] if k % 2 else None, o[2], o[3] if k % 4 < 2 else None, o[4])
            return self.grab(0, 1, 2, 3, 4)
        if op == "packetFrameInfo":
            return obs(e.packetFrameInfo())

        # ---- setters that invalidate state ----
        if op == "setRecordFormat":
            e.setRecordFormat(pkg.RECORDS_PACKED48 if k % 2 else pkg.RECORDS_F64); return e.getRecordFormat()
        if op == "setRegularizationPose":
            e.setRegularizationScaleFactor(0.0 if k % 3 == 0 else 0.01); e.setRegularizationPose(self.lend(guesses[(k + 1) % 3])); return "ok"
        if op == "unsetRegularizationPose":
            e.unsetRegularizationPose(); return "ok"
        if op == "setTransformationEpsilon":
            e.setTransformationEpsilon(1e-3 if k % 2 else 1e-4); return "ok"
        if op == "setOutlierRatio":                           # (the Gauss constants of every later evaluation)
            e.setOutlierRatio(0.4 if k % 2 else 0.55); return "ok"
        if op == "setMinPointPerVoxel":                       # a grid parameter: a kept cloud is re-voxelised, any other target dropped
            e.setMinPointPerVoxel(4 if k % 2 else 6); return self.call(e, "grid", 0)
        if op == "sourceChanged":
            # the caller's scan buffer, viewed by the engine, rewritten in place (both engines view the same arrays: the
            # second rewrite of a step writes what is there already)
            c = sources[k % 3][:self.view_n]
            for ax in range(3):
                hip.write(self.view[ax], np.ascontiguousarray(c[:, ax]))
            if k % 4 < 2:
                e.setInputSourceDeviceView(self.view[0], self.view[1], self.view[2], self.view_n)
            e.sourceChanged()
            return self.call(e, "score", k)
        raise AssertionError(op)


@pytest.fixture()
def rig(pkg, S, hipmem):
    r = Rig(pkg, S, hipmem)
    r.eng = [r.engine(pkg.HANDOFF_SYNC), r.engine(pkg.HANDOFF_ASYNC)]
    for e in r.eng:   # two builds of the largest cloud: the index capacity is final, every later build is steady state
        e.setInputTarget(r.hull); e.wait()
        e.setInputTarget(r.hull); e.wait()
    yield r
    for e in r.eng:
        e.close()


def both(rig, op, k):
    """The op on the blocking engine, then on the asynchronous one; for a target call the blocking engine refuses at once
    and the asynchronous one defers, the verdict is taken with wait()."""
    ra = rig.call(rig.eng[0], op, k)
    rb = rig.call(rig.eng[1], op, k)
    deferred = False
    if (op.startswith("target") or op.startswith("setInputTargetFrom")) and isinstance(ra, tuple) and ra[0] == "error" and rb == "ok":
        deferred = True
        rb = rig.call(rig.eng[1], "wait", 0)
    return ra, rb, deferred


def bucket_sum(e):
    c = e.buildCounters()
    return c[1] + c[2]


# ---- 2. the matrix ----------------------------------------------------------------------------------------------------
# every op added here as a consumer, k = 0 .. 3 (the argument variants that take different paths) and the few beyond
VARIANTS = {"mapReset": (0, 1, 3, 7), "mapImportState": (1, 2, 4), "putKeyframe": (0, 3, 4, 7), "setInputTargetFromKeyframes": (0, 1, 2, 3, 4),
            "filterSource": (0, 1, 2, 3, 4, 5)}
CONSUMERS = [(op, k) for op in NEW_OPS for k in VARIANTS.get(op, (0, 1, 2, 3))]


@pytest.mark.parametrize("producer", list(PRODUCERS))
def test_producer_then_consumer_async_equals_sync(rig, producer):
    """P then C with nothing in between, for every op of this file as C (k = 0 .. 3 each and a few beyond: CONSUMERS), then
    one align;
    the asynchronous engine's build at a target producer was the steady-state kind (see the module's docstring)."""
    t0 = time.perf_counter()
    p_op, p_k = PRODUCERS[producer]
    a, b = rig.eng
    if producer in TARGET_PRODUCERS:   # the producer's build alone, collected by wait(): one more two-launch build
        rig.prepare(b)
        before = bucket_sum(b)
        assert rig.call(b, p_op, p_k) == "ok" and rig.call(b, "wait", 0) == "ok"
        assert bucket_sum(b) == before + 1, "%s(%d) was not a steady-state two-launch build: %s" % (p_op, p_k, b.buildCounters())
    for c_op, c_k in CONSUMERS:
        what = "%s(%d) then %s(%d)" % (p_op, p_k, c_op, c_k)
        for e in rig.eng:
            rig.prepare(e)
        before = [bucket_sum(e) for e in rig.eng]
        pa = rig.call(a, p_op, p_k)
        pb = rig.call(b, p_op, p_k)
        if producer in TARGET_PRODUCERS:
            # (the counters move when a build's verdict is collected: at once on the blocking engine, and on the
            # asynchronous one not before the consumer -- the build is in flight when the consumer is called)
            assert pa == pb == "ok", what
            assert bucket_sum(a) == before[0] + 1, "%s: not a steady-state two-launch build on the blocking engine: %s" % (
                what, a.buildCounters())
            assert bucket_sum(b) == before[1], "%s: the asynchronous engine's build was not left pending: %s" % (what, b.buildCounters())
        elif producer == "target_bad":
            assert pa == ("error", -4) and pb == "ok", "%s: the failing build was not left pending (%s, %s)" % (what, pa, pb)
        else:
            assert pa == pb, what
        ra, rb, _ = both(rig, c_op, c_k)
        assert ra == rb, "%s: blocking %s, asynchronous %s" % (what, brief(ra), brief(rb))
        ra, rb = rig.call(a, "align", 0), rig.call(b, "align", 0)
        assert ra == rb, "%s, then align: blocking %s, asynchronous %s" % (what, brief(ra), brief(rb))
        if producer in TARGET_PRODUCERS:   # collected by now: the same two-launch builds on both engines, the producer's among them
            grown = [bucket_sum(e) - n for e, n in zip(rig.eng, before)]
            assert grown[1] == grown[0] >= 1, "%s: two-launch builds %s" % (what, grown)
    print("matrix[%s]: %d pairs in %.2f s" % (producer, len(CONSUMERS), time.perf_counter() - t0))


def test_deferred_failure_survives_keep_grid_calls_and_is_reported_once(rig):
    """The failing producer, then a keep-grid consumer (same observation as on the blocking engine, which heard of the
    failure from its target call), then a call that needs the grid: on the asynchronous engine it fails with exactly the
    code -- and the text -- of the blocking engine's target call; the call after that finds no target on both."""
    t0 = time.perf_counter()
    a, b = rig.eng
    for c_op, c_k in KEEP_GRID_CONSUMERS:
        for g_op, g_k in GRID_CONSUMERS:
            what = "target_bad then %s(%d) then %s" % (c_op, c_k, g_op)
            for e in rig.eng:
                rig.prepare(e)
            pa, pb = rig.call(a, "target_bad", 0), rig.call(b, "target_bad", 0)
            verdict = rig.messages[a.tag]
            assert pa == ("error", -4) and "finite" in verdict and pb == "ok", (what, pa, pb)
            ra, rb = rig.call(a, c_op, c_k), rig.call(b, c_op, c_k)
            assert ra == rb and not refused(ra), "%s: blocking %s, asynchronous %s" % (
                what, brief(ra), brief(rb))
            rig.messages.pop(b.tag, None)
            ga, gb = rig.call(a, g_op, g_k), rig.call(b, g_op, g_k)
            assert gb == pa, "%s: the asynchronous engine answered %s" % (what, brief(gb))
            # (the build's verdict and "no target" are the same status, NDT_ERR_NO_TARGET: which of the two a call reports
            # shows in the text alone -- the build's "target has no finite point", word for word what the blocking engine's
            # target call said; the fitness index has a "no finite point" text of its own, which a handle without a grid
            # never reaches)
            assert rig.messages[b.tag] == verdict and "finite" in verdict, (what, rig.messages[b.tag], verdict)
            assert ga == ("error", -4) and "finite" not in rig.messages[a.tag], (what, ga, rig.messages[a.tag])
            na, nb = rig.call(a, g_op, g_k), rig.call(b, g_op, g_k)
            assert na == nb == ("error", -4) and "finite" not in rig.messages[b.tag], (what, na, nb, rig.messages[b.tag])
            for e in rig.eng:
                e.wait()
    print("deferred failures: %.2f s" % (time.perf_counter() - t0))


def test_resolution_change_on_a_union_drops_it_instead_of_rebuilding_a_stale_cloud(rig):
    """Found by a random sequence of this vocabulary before its last three setters were added (on BOTH engines alike: a
    GPU memory fault, not a mismatch) and reduced: tiles added, then a small host target (the engine keeps its
    cloud), then createVoxelKdtree -- which counted the tiles' 5 808 points as the target's while the 1 334-point cloud stayed
    --, then setResolution:
    ndt_set_params re-voxelised `n_target_points` points of the kept cloud, reading past its end.  A union cannot be
    re-voxelised (its tiles were built with the old parameters): like a consumed device target it is dropped, the next
    consumer finds no target, and createVoxelKdtree is refused until the tiles have been added again."""
    seq = [("addTarget", 0), ("addTarget", 1), ("addTarget", 2), ("target", 2), ("createVoxelKdtree", 0), ("grid", 0), ("align", 0),
           ("resolution", 0), ("grid", 0), ("align", 0), ("leaves", 0), ("createVoxelKdtree", 0), ("resolution", 1),
           ("createVoxelKdtree", 0), ("grid", 0), ("align", 0)]
    for e in rig.eng:
        rig.prepare(e)
    seen = []
    for i, (op, k) in enumerate(seq):
        ra, rb, _ = both(rig, op, k)
        assert ra == rb, "step %d %s(%d): blocking %s, asynchronous %s" % (i, op, k, brief(ra), brief(rb))
        seen.append(ra)
    assert len(rig.clouds[2]) < sum(len(t) for t in rig.tiles)          # (the kept cloud is the smaller one)
    assert not refused(seen[4]) and not refused(seen[5]) and not refused(seen[6])
    assert seen[8] == seen[9] == seen[10] == ("error", -4)              # no target after the resolution change
    assert seen[11] == ("error", -1)                                    # tiles of the other resolution
    assert seen[13] == seen[4] and seen[14] == seen[5] and seen[15] == seen[6]


# ---- 3. random sequences ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS + extra_seeds())
def test_random_full_api_sequences_async_equals_sync(rig, seed):
    t0 = time.perf_counter()
    for e in rig.eng:
        rig.prepare(e)
    history, served, n_served, deferred = [], set(), 0, 0
    for i, (op, k) in enumerate(sequence(seed)):
        history.append((op, k))
        ra, rb, late = both(rig, op, k)
        assert ra == rb, "seed %d step %d, last calls %s: blocking %s, asynchronous %s" % (
            seed, i, " ".join("%s(%d)" % h for h in history[-10:]), brief(ra), brief(rb))
        deferred += late
        if not refused(ra):
            served.add(op)
            n_served += 1
    print("sequence[%d]: %d calls in %.2f s, %d served, never served %s, %d deferred verdicts, asynchronous engine: builds %s, "
          "speculation %s" % (seed, len(history), time.perf_counter() - t0, n_served, sorted(set(OPS) - served), deferred,
                              rig.eng[1].buildCounters(), rig.eng[1].speculationCounters()))
    if seed in SEEDS:
        # not a sequence of refusals (a refusal compares one status code; more than half of the calls must have done their
        # work), and failing builds were left pending on the asynchronous engine
        assert 2 * n_served > len(history) and deferred >= 3


# ---- 4. the transition table ------------------------------------------------------------------------------------------
NO_TARGET, UNSUPPORTED = -4, -9
# producer (op, k) -> does the engine keep the cloud the grid was built from
TABLE_PRODUCERS = [("target", 1, True), ("target_xyzi", 2, True), ("target_soa", 3, True), ("target_dev", 0, False),
                   ("target_dev_deferred", 3, False), ("setInputTargetFromKeyframes", 1, True), ("setInputTargetFromMap", 0, True),
                   ("setInputTargetFromMapMoments", 1, False), ("addTarget", 2, False), ("createVoxelKdtree", 0, False)]
TABLE_INVALIDATORS = [("resolution", 0), ("setMinPointPerVoxel", 1), ("removeTarget", 0), ("addTarget", 2), ("target_bad", 0)]


class TargetModel:
    """What the engine's target is after a call, restated: kind NONE | SINGLE | UNION, whether the cloud is kept, the
    points it reports; the tiles stored for a union and the two grid parameters the invalidators change."""

    def __init__(self, rig, e):
        self.rig, self.kind, self.cloud, self.points = rig, "NONE", False, 0
        self.tiles = {11: len(rig.tiles[0]), 12: len(rig.tiles[1])}
        self.res, self.min_pts = 1.0, 6
        # what the map-made targets stand for: every voxel's centroid / every point of the map's voxels (the whole map is
        # selected: what setInputTarget would build from every point ever added)
        self.map_voxels = e.mapInfo()["n_voxels"]
        self.map_moment_points = int(e.mapExport(with_counts=True)[1].sum())

    def apply(self, op, k):
        rig = self.rig
        single = lambda cloud, points: ("SINGLE", cloud, points)   # noqa: E731
        if op in ("target", "target_xyzi", "target_soa"):
            self.kind, self.cloud, self.points = single(True, len(rig.clouds[k % 4]))
        elif op in ("target_dev", "target_dev_deferred"):
            self.kind, self.cloud, self.points = single(False, len(rig.clouds[k % 4]))
        elif op == "setInputTargetFromKeyframes":
            assert k == 1
            self.kind, self.cloud, self.points = single(True, len(rig.kf_clouds[0]) + len(rig.kf_clouds[1]))
        elif op == "setInputTargetFromMap":
            assert k == 0
            self.kind, self.cloud, self.points = single(True, self.map_voxels)
        elif op == "setInputTargetFromMapMoments":
            assert k == 1
            self.kind, self.cloud, self.points = single(False, self.map_moment_points)
        elif op == "addTarget":
            self.tiles[11 + k % 3] = len(rig.tiles[k % 3])
            self.kind, self.cloud, self.points = "NONE", False, 0
        elif op == "createVoxelKdtree":
            self.kind, self.cloud, self.points = "UNION", False, sum(self.tiles.values())
        elif op in ("resolution", "setMinPointPerVoxel"):
            if op == "resolution":
                self.res = 1.0 if k % 2 else 1.5
            else:
                self.min_pts = 4 if k % 2 else 6
            if not (self.kind == "SINGLE" and self.cloud):       # a kept cloud is re-voxelised, anything else is dropped
                self.kind, self.points = "NONE", 0
        elif op == "removeTarget":
            del self.tiles[11 + k % 3]
            if self.kind == "UNION":
                self.kind, self.points = "NONE", 0
        elif op == "target_bad":
            self.kind, self.cloud, self.points = "NONE", False, 0
        else:
            raise AssertionError(op)


def status(r):
    return r[1] if refused(r) else 0


def table_reset(rig, e):
    """NONE, no cloud, two tiles stored at the parameters in force, every grid parameter where prepare() left it"""
    e.setParams(resolution=1.0, min_points_per_voxel=6, max_iterations=2)   # (the statuses are what is asserted: a short align)
    rig.call(e, "removeTarget", 2)
    assert rig.call(e, "addTarget", 0) == rig.call(e, "addTarget", 1) == 2


def table_check(rig, e, m, what):
    """the public binding against the model; returns (grid, leaves) as observations"""
    grid, leaves = rig.call(e, "grid", 0), rig.call(e, "leaves", 0)
    seen = dict(grid=status(grid), leaves=status(leaves), align=status(rig.call(e, "align", 0)), fitness=status(rig.call(e, "fitness", 0)))
    if m.kind == "NONE":
        assert seen == dict(grid=NO_TARGET, leaves=NO_TARGET, align=NO_TARGET, fitness=NO_TARGET), (what, e.tag, seen)
        return grid, leaves
    g = e.getGridInfo()
    # (align needs one valid voxel, as the C-ABI documents NDT_ERR_NO_TARGET: the map's centroids, one point a voxel at
    # its own leaf, make a grid without one)
    want = dict(grid=0, leaves=0, align=0 if g["n_leaves"] > 0 else NO_TARGET,
                fitness=0 if m.kind == "SINGLE" and m.cloud else UNSUPPORTED)
    assert seen == want, (what, e.tag, m.kind, m.cloud, seen, want)
    assert g["n_target_points"] == m.points and g["leaf_size"] == np.float32(m.res), (what, e.tag, g, m.points, m.res)
    return grid, leaves


def test_target_transition_table(rig):
    """Every producer, then every invalidator, on both engines: the state each leaves (the tables of the issue that
    introduced csrc/ndt_target_state.*, derived from the code before it and passing there unchanged).  A resolution or
    min-points change on a SINGLE with its cloud rebuilds it: grid info and leaves equal, bit for bit, what a third engine
    that never saw the old parameters builds from the same producer at the new ones."""
    t0 = time.perf_counter()
    pkg = rig.pkg
    ref = rig.engine(pkg.HANDOFF_SYNC)
    ref.tag = "reference"
    try:
        for e in rig.eng + [ref]:
            rig.prepare(e)
        fresh = {}

        def reference(p_op, p_k, i_op, i_k):
            key = (p_op, p_k, i_op, i_k)
            if key not in fresh:
                table_reset(rig, ref)
                assert rig.call(ref, i_op, i_k) is not None           # the new parameter first, on a handle without a target
                assert rig.call(ref, p_op, p_k) == "ok"
                fresh[key] = (rig.call(ref, "grid", 0), rig.call(ref, "leaves", 0))
                assert not refused(fresh[key][0]) and not refused(fresh[key][1])
            return fresh[key]

        n = 0
        for e in rig.eng:
            for p_op, p_k, keeps in TABLE_PRODUCERS:
                for i_op, i_k in TABLE_INVALIDATORS:
                    what = "%s(%d) then %s(%d)" % (p_op, p_k, i_op, i_k)
                    table_reset(rig, e)
                    m = TargetModel(rig, e)
                    table_check(rig, e, m, "reset before " + what)
                    r = rig.call(e, p_op, p_k)
                    assert not refused(r), (what, e.tag, r)
                    m.apply(p_op, p_k)
                    assert m.cloud == keeps
                    before = table_check(rig, e, m, what + ": after the producer")
                    was = m.kind
                    r = rig.call(e, i_op, i_k)
                    if i_op == "target_bad":
                        # refused at once, or -- the asynchronous engine in steady state, which a union's whole-index fill
                        # ends -- left pending and reported by the next consumer
                        assert r == ("error", NO_TARGET) or (r == "ok" and e is rig.eng[1]), (what, e.tag, r)
                    else:
                        assert not refused(r) or i_op == "setMinPointPerVoxel", (what, e.tag, r)
                    m.apply(i_op, i_k)
                    after = table_check(rig, e, m, what)
                    if i_op in ("resolution", "setMinPointPerVoxel") and m.kind == "SINGLE":
                        assert after == reference(p_op, p_k, i_op, i_k), "%s on the %s engine: the rebuilt grid is not the fresh one" % (what, e.tag)
                    if i_op == "removeTarget" and was != "UNION":
                        assert after == before, "%s on the %s engine: removeTarget touched a target that is no union" % (what, e.tag)
                    n += 1
        assert n == 2 * len(TABLE_PRODUCERS) * len(TABLE_INVALIDATORS)
    finally:
        ref.close()
    print("transition table: %d producer-invalidator pairs in %.2f s" % (n, time.perf_counter() - t0))
