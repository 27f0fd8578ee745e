"""The deskew model on the host: ndt_trajectory_pose against a NumPy f64 reference that is deliberately NOT the product's
formula -- the rotation of segment k at u is R_k Exp(u Log(R_k^T R_{k+1})) (synth.so3_log + Rodrigues: the same geodesic
the product walks with a quaternion slerp), the translation the linear blend of d_k -- the rigid-segment rule, every
refusal, the host code under AddressSanitizer + UBSan as a stand-alone program, and the kernels' scratch use.  No GPU.
The reference and the trajectory generator are shared with tests/test_gpu_deskew.py."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1

# rotation of one segment: below the slerp's linear-blend threshold, small (what acos of a dot product would lose), typical,
# and large
SEGMENT_ROTATIONS = [1e-10, 1e-5, np.deg2rad(3.0), np.deg2rad(90.0), np.deg2rad(170.0)]
KNOT_COUNTS = [1, 2, 3, 64]


# --------------------------------------------------------------------------- the reference
def rodrigues(axis, th):
    """R = I + sin(th) K + 2 sin^2(th / 2) K^2 for a unit axis; th: scalar or [m] -> [3, 3] or [m, 3, 3]."""
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    th = np.asarray(th, np.float64)
    s, c1 = np.sin(th)[..., None, None], (2.0 * np.sin(0.5 * th) ** 2)[..., None, None]
    return np.eye(3) + s * K + c1 * (K @ K)


def inv_pose(T):
    T = np.asarray(T, np.float64)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def reduce_knots(knot_poses, ref_pose=None):
    """D_k = ref^-1 T_k, ref None = the last knot."""
    kp = np.asarray(knot_poses, np.float64)
    ref = kp[-1] if ref_pose is None else np.asarray(ref_pose, np.float64)
    return np.stack([inv_pose(ref) @ T for T in kp])


def segment_index(knot_t, t):
    """t (clamped) -> k with knot_t[k] <= t <= knot_t[k + 1]; at an interior knot either neighbour gives the same pose."""
    n = len(knot_t)
    return np.clip(np.searchsorted(knot_t, t, side="right") - 1, 0, max(n - 2, 0))


def pose_numpy(S, knot_t, knot_poses, t, ref_pose=None):
    """D(t) as a 4 x 4 f64 matrix."""
    knot_t = np.asarray(knot_t, np.float64)
    D = reduce_knots(knot_poses, ref_pose)
    if len(knot_t) == 1:
        return D[0]
    t = min(max(float(t), knot_t[0]), knot_t[-1])
    k = int(segment_index(knot_t, t))
    u = (t - knot_t[k]) / (knot_t[k + 1] - knot_t[k])
    w = S.so3_log(D[k][:3, :3].T @ D[k + 1][:3, :3])
    th = np.linalg.norm(w)
    out = np.eye(4)
    out[:3, :3] = D[k][:3, :3] @ (rodrigues(w / th, u * th) if th > 0.0 else np.eye(3))
    out[:3, 3] = D[k][:3, 3] + u * (D[k + 1][:3, 3] - D[k][:3, 3])
    return out


def poses_numpy(S, knot_t, knot_poses, t, ref_pose=None):
    """D(t_i) for an array of (finite) times: (R [m, 3, 3], d [m, 3])."""
    knot_t = np.asarray(knot_t, np.float64)
    D = reduce_knots(knot_poses, ref_pose)
    t = np.asarray(t, np.float64)
    R = np.broadcast_to(D[0][:3, :3], (len(t), 3, 3)).copy()
    d = np.broadcast_to(D[0][:3, 3], (len(t), 3)).copy()
    if len(knot_t) == 1:
        return R, d
    tc = np.clip(t, knot_t[0], knot_t[-1])
    seg = segment_index(knot_t, tc)
    for k in range(len(knot_t) - 1):
        m = seg == k
        if not m.any():
            continue
        u = (tc[m] - knot_t[k]) / (knot_t[k + 1] - knot_t[k])
        w = S.so3_log(D[k][:3, :3].T @ D[k + 1][:3, :3])
        th = np.linalg.norm(w)
        Ru = rodrigues(w / th, u * th) if th > 0.0 else np.broadcast_to(np.eye(3), (len(u), 3, 3))
        R[m] = D[k][:3, :3] @ Ru
        d[m] = D[k][:3, 3] + u[:, None] * (D[k + 1][:3, 3] - D[k][:3, 3])
    return R, d


def deskew_numpy(S, pts, t, knot_t, knot_poses, ref_pose=None):
    """[n, 3] f64: the f32 points moved by D(t_i) in f64 (not rounded); non-finite points give NaN."""
    p = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
    tt = np.asarray(t, np.float32).astype(np.float64)
    out = np.full((len(p), 3), np.nan)
    ok = np.isfinite(p).all(1) & np.isfinite(tt)
    R, d = poses_numpy(S, knot_t, knot_poses, tt[ok], ref_pose)
    out[ok] = np.einsum("mij,mj->mi", R, p[ok]) + d
    return out


def ulp_f32(v):
    """Spacing of float32 at |v| (v: f64), from v's own binade (not from its rounded value)."""
    e = np.frexp(np.abs(np.asarray(v, np.float64)))[1]          # |v| in [2^(e-1), 2^e)
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def assert_points_within_tolerance(out, ref64, what=""):
    """|out - ref64| <= 0.5 ulp_f32(|ref64|) + 1e-9 m per coordinate, every point; NaN where the reference is NaN."""
    out = np.asarray(out, np.float64)
    assert out.shape == ref64.shape, (what, out.shape, ref64.shape)
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(out), nan), what
    err = np.abs(out - ref64)[~nan]
    bound = 0.5 * ulp_f32(ref64[~nan]) + 1e-9
    worst = float((err / bound).max()) if err.size else 0.0
    assert worst <= 1.0, "%s: %d coordinates beyond the bound, worst %.3f x" % (what, int((err > bound).sum()), worst)


# --------------------------------------------------------------------------- trajectories
def random_rotation(rng):
    ax = rng.normal(size=3)
    return rodrigues(ax / np.linalg.norm(ax), rng.uniform(0.0, np.pi))


def make_trajectory(n_knots, seed, rotations=SEGMENT_ROTATIONS, t0=0.0, step=0.1, trans=1.0):
    """(knot_t [n], knot_poses [n, 4, 4]): a random start pose, then segment k turns by rotations[k % len] about a random
    axis and moves by up to `trans` m; knot times increase by random steps around `step`."""
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, :3] = random_rotation(rng)
    T[:3, 3] = rng.uniform(-50.0, 50.0, 3)
    poses, times, t = [T.copy()], [t0], t0
    for k in range(n_knots - 1):
        ax = rng.normal(size=3)
        d = np.eye(4)
        d[:3, :3] = rodrigues(ax / np.linalg.norm(ax), rotations[k % len(rotations)])
        d[:3, 3] = rng.uniform(-trans, trans, 3)
        T = T @ d
        t += step * rng.uniform(0.5, 1.5)
        poses.append(T.copy())
        times.append(t)
    return np.array(times), np.stack(poses)


def probe_times(knot_t):
    """every knot, every mid-segment, below and above the ends"""
    knot_t = np.asarray(knot_t, np.float64)
    span = max(knot_t[-1] - knot_t[0], 1.0)
    mids = 0.5 * (knot_t[:-1] + knot_t[1:])
    thirds = knot_t[:-1] + 0.3 * (knot_t[1:] - knot_t[:-1])
    return np.concatenate([knot_t, mids, thirds, [knot_t[0] - 0.5 * span, knot_t[-1] + 0.5 * span]])


def ref_choices(knot_poses, seed):
    rng = np.random.default_rng(seed + 1000)
    other = np.eye(4)
    other[:3, :3] = random_rotation(rng)
    other[:3, 3] = knot_poses[0][:3, 3] + rng.uniform(-3.0, 3.0, 3)
    return [("last", None), ("first", knot_poses[0]), ("other", other)]


# --------------------------------------------------------------------------- ndt_trajectory_pose
@pytest.mark.parametrize("n_knots", KNOT_COUNTS)
def test_trajectory_pose_matches_the_geodesic_reference(pkg, S, n_knots):
    for seed in range(3):
        # (every segment rotation in first place once: n_knots = 2 has a single segment)
        rots = SEGMENT_ROTATIONS[seed:] + SEGMENT_ROTATIONS[:seed]
        for first in range(len(rots) if n_knots == 2 else 1):
            kt, kp = make_trajectory(n_knots, 10 * seed + first, rots[first:] + rots[:first])
            for name, ref in ref_choices(kp, seed):
                for t in probe_times(kt):
                    got = pkg.trajectory_pose(kt, kp, t, ref)
                    want = pose_numpy(S, kt, kp, t, ref)
                    assert np.array_equal(got[3], [0.0, 0.0, 0.0, 1.0])
                    assert np.abs(got[:3, :3] - want[:3, :3]).max() <= 1e-12, (n_knots, seed, name, t)
                    assert np.all(np.abs(got[:3, 3] - want[:3, 3]) <= 1e-12 * (1.0 + np.abs(want[:3, 3]))), (n_knots, seed, name, t)


def test_trajectory_pose_clamps_outside_the_knots(pkg):
    kt, kp = make_trajectory(3, 5)
    assert np.array_equal(pkg.trajectory_pose(kt, kp, kt[0] - 7.0), pkg.trajectory_pose(kt, kp, kt[0]))
    assert np.array_equal(pkg.trajectory_pose(kt, kp, kt[-1] + 7.0), pkg.trajectory_pose(kt, kp, kt[-1]))


def test_rigid_segments_are_exact(pkg):
    kt, kp = make_trajectory(4, 9)
    kp[2] = kp[1]                                     # segment [1, 2] does not move
    for ref in (None, kp[0], kp[1]):
        at_knot = pkg.trajectory_pose(kt, kp, kt[1], ref)
        for u in (0.0, 1e-9, 0.25, 0.5, 1.0 / 3.0, 0.999, 1.0):
            t = kt[1] + u * (kt[2] - kt[1])
            assert pkg.trajectory_pose(kt, kp, t, ref).tobytes() == at_knot.tobytes(), (u,)
    # every knot equal to the reference: the identity, exactly -- whatever the pose is
    for n in (1, 2, 5, 64):
        _, one = make_trajectory(1, 40 + n)
        same = np.repeat(one, n, axis=0)
        times = np.arange(n, dtype=np.float64)
        for ref in (None, one[0]):
            for t in probe_times(times):
                assert pkg.trajectory_pose(times, same, t, ref).tobytes() == np.eye(4).tobytes(), (n, t)


def test_trajectory_pose_refusals(pkg):
    import ctypes as C
    L = pkg.lib()
    kt, kp = make_trajectory(3, 2)
    poses = np.ascontiguousarray(np.transpose(kp, (0, 2, 1))).ravel()
    out = np.zeros(16)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731

    def call(times=kt, p=poses, n=3, ref=None, t=0.05, o=out):
        return L.ndt_trajectory_pose(None if times is None else dp(times), None if p is None else dp(p), n,
                                     None if ref is None else dp(ref), t, None if o is None else dp(o))

    assert call(times=None) == INVALID_ARG and call(p=None) == INVALID_ARG and call(o=None) == INVALID_ARG
    big_t, big_p = make_trajectory(65, 3)
    big_p = np.ascontiguousarray(np.transpose(big_p, (0, 2, 1))).ravel()
    assert call(times=big_t, p=big_p, n=64) == 0
    assert call() == 0
    written = out.copy()
    assert call(times=big_t, p=big_p, n=65) == INVALID_ARG
    assert call(n=0) == INVALID_ARG and call(n=-1) == INVALID_ARG
    assert call(times=np.array([0.0, 0.2, 0.1])) == INVALID_ARG          # not increasing
    assert call(times=np.array([0.0, 0.1, 0.1])) == INVALID_ARG          # not STRICTLY increasing
    for bad in (np.nan, np.inf, -np.inf):
        assert call(times=np.array([0.0, 0.1, bad])) == INVALID_ARG
        assert call(times=np.array([bad, 0.1, 0.2])) == INVALID_ARG
        assert call(t=bad) == INVALID_ARG
        for e in (0, 5, 12, 15, 16 + 13, 47):
            p = poses.copy()
            p[e] = bad
            assert call(p=p) == INVALID_ARG, (bad, e)
        r = poses[:16].copy()
        r[14] = bad
        assert call(ref=r) == INVALID_ARG
    assert np.array_equal(out, written) and np.array_equal(out, pkg.trajectory_pose(kt, kp, 0.05).T.ravel())   # refused: nothing written
    with pytest.raises(pkg.NdtError):
        pkg.trajectory_pose([0.0, 0.0], kp[:2], 0.0)
    with pytest.raises(ValueError):
        pkg.trajectory_pose(kt, kp[:2], 0.0)


def test_scan_filter_from_vehicle_box(pkg):
    f = pkg.ScanFilter()
    assert bytes(f) == bytes(C_sizeof(pkg)) and not f.use_box and not f.use_z_or_intensity
    f = pkg.ScanFilter.from_vehicle_box([1.0, 0.0, -0.5], [4.0, 2.0, 1.0], z_band=(-2.0, 3.0), intensity_keep_min=40.0)
    assert f.use_box == 1 and list(f.box_min) == [-1.0, -1.0, -1.0] and list(f.box_max) == [3.0, 1.0, 0.0]
    assert f.use_z_or_intensity == 1 and (f.z_min, f.z_max, f.intensity_keep_min) == (-2.0, 3.0, 40.0)
    f = pkg.ScanFilter.from_vehicle_box(None, None, z_band=(0.0, 1.0))
    assert f.use_box == 0 and f.use_z_or_intensity == 1 and f.intensity_keep_min == np.inf


def C_sizeof(pkg):
    import ctypes as C
    assert C.sizeof(pkg.ScanFilter) == 44   # int, 6 floats, int, 3 floats: the struct of include/ndt_hip.h
    return C.sizeof(pkg.ScanFilter)


# --------------------------------------------------------------------------- sanitizers, stand-alone
def test_trajectory_host_code_under_asan_ubsan(tmp_path):
    """tests/cpp/sanitize_trajectory.cpp (its own main) + csrc/ndt_trajectory.cpp under ASan + UBSan as a child process:
    the same knot counts, segment rotations and probe times as above, plus the refusals.  Never through Python's loader."""
    exe = str(tmp_path / "sanitize_trajectory")
    csrc = os.path.join(ROOT, "slam-sam_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                        "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                        os.path.join(ROOT, "tests", "cpp", "sanitize_trajectory.cpp"), os.path.join(csrc, "ndt_trajectory.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("PASS"), r.stdout[-2000:]


# --------------------------------------------------------------------------- kernel resources
def test_deskew_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_deskew.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "d.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", ln)
        if m and name and "k_deskew" in name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    kernels = sorted(re.search(r"k_deskew_[a-z]+", n).group(0) for n in usage)
    assert kernels == ["k_deskew_aligned", "k_deskew_count", "k_deskew_emit"], sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
