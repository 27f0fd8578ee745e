"""Seeded, dependency-free synthetic clouds for the NDT configurations of BASELINE.json.

Nothing here reads the reference tree; the geometry follows SURVEY.md section 8(d):
  * two_planes(): the reference test's two-plane fixture
    (ref: extern/svn_ndt/test/test_svn_ndt.cpp:44-83) with a portable PRNG;
  * OusterSim: ray-cast OS-2-128-style scans (128 or 256 beams x 1024 columns,
    +-11.25 deg vertical FOV, range clipped to [0.5, 250] m as
    config/lidar_config_berlin.json does) inside a seeded block-world street scene;
  * config_c1 / config_c2 / config_c3: the workloads C1, C2 and C3/C4.
All functions return float32 N x 3 arrays and float64 4x4 poses.
"""
import numpy as np


# --------------------------------------------------------------------------- poses
def rot_xyz(roll, pitch, yaw):
    """R = Rx(roll) Ry(pitch) Rz(yaw) (the NDT pose convention)."""
    cx, sx, cy, sy, cz, sz = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def pose_matrix(x, y, z, roll, pitch, yaw):
    T = np.eye(4)
    T[:3, :3] = rot_xyz(roll, pitch, yaw)
    T[:3, 3] = [x, y, z]
    return T


def so3_log(R):
    """Rotation vector of R; atan2 form so tiny angles do not underflow to zero."""
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(a)
    c = (np.trace(R) - 1.0) / 2.0
    th = np.arctan2(s, c)
    if s < 1e-300:
        return np.zeros(3)
    return a * (th / s)


def pose_error(T_est, T_ref):
    """(translation error in m, rotation error in rad) of inv(T_est) @ T_ref."""
    E = np.linalg.inv(np.asarray(T_est, dtype=np.float64)) @ np.asarray(T_ref, dtype=np.float64)
    return float(np.linalg.norm(E[:3, 3])), float(np.linalg.norm(so3_log(E[:3, :3])))


def se3_log_error(T_est, T_ref):
    """Norms of the rotation / translation parts of Log(inv(T_est) T_ref), the metric of
    the reference test (ref: test_svn_ndt.cpp:188-191)."""
    E = np.linalg.inv(np.asarray(T_est, dtype=np.float64)) @ np.asarray(T_ref, dtype=np.float64)
    w = so3_log(E[:3, :3])
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-9:
        Vinv = np.eye(3) - 0.5 * K
    else:
        Vinv = np.eye(3) - 0.5 * K + (1.0 / th ** 2) * (1.0 - th * np.sin(th) / (2.0 * (1.0 - np.cos(th)))) * (K @ K)
    u = Vinv @ E[:3, 3]
    return float(np.linalg.norm(u)), float(th)


def transform(T, pts):
    T = np.asarray(T, dtype=np.float64)
    return (pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


# --------------------------------------------------------------------------- two planes
def two_planes(seed=1337, noise=0.02, step=0.15, half=10.0, max_points=None):
    """Source / target / ground truth / initial guess of the reference test geometry."""
    rng = np.random.default_rng(seed)
    ax = np.arange(-half, half + 1e-9, step)
    gx, gy = np.meshgrid(ax, ax, indexing="ij")
    p1 = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1)
    p2 = np.stack([gx.ravel(), np.zeros(gx.size), gy.ravel()], 1)
    src = np.concatenate([p1, p2]).astype(np.float32)
    if max_points is not None and len(src) > max_points:
        sel = np.sort(rng.choice(len(src), size=max_points, replace=False))
        src = src[sel]
    # ground truth Rz(0.2618) Ry(0.0873), t = (0.5, 0, 0.3)  (ref :104-106)
    cz, sz, cy, sy = np.cos(0.2618), np.sin(0.2618), np.cos(0.0873), np.sin(0.0873)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    gt = np.eye(4)
    gt[:3, :3] = Rz @ Ry
    gt[:3, 3] = [0.5, 0.0, 0.3]
    tgt = (src.astype(np.float64) @ gt[:3, :3].T + gt[:3, 3] + rng.normal(0.0, noise, src.shape)).astype(np.float32)
    # initial guess: gt * Exp(-delta), delta = [rot 0.05,-0.02,0.04 | trans 0.02,-0.01,0.03] (ref :110-111)
    w = -np.array([0.05, -0.02, 0.04])
    v = -np.array([0.02, -0.01, 0.03])
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    dR = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * (K @ K)
    d = np.eye(4)
    d[:3, :3] = dR
    d[:3, 3] = V @ v
    guess = gt @ d
    return src, tgt, gt, guess


# --------------------------------------------------------------------------- lidar sim
class Scene:
    """Ground plane z = 0, axis-aligned boxes, and an enclosing wall box."""

    def __init__(self, seed=42, extent=(120.0, 80.0), n_boxes=60, wall_height=30.0):
        rng = np.random.default_rng(seed)
        ex, ey = extent
        boxes = []
        # two rows of buildings along a street (the x axis), plus scattered blocks
        x = -ex
        while x < ex:
            w = rng.uniform(8.0, 25.0)
            for side in (-1, 1):
                d = rng.uniform(8.0, 20.0)
                hgt = rng.uniform(6.0, 25.0)
                y0 = side * rng.uniform(7.0, 10.0)
                y1 = y0 + side * d
                boxes.append([x, min(y0, y1), 0.0, x + w - rng.uniform(0.5, 3.0), max(y0, y1), hgt])
            x += w
        for _ in range(n_boxes):
            cx, cy = rng.uniform(-ex, ex), rng.uniform(-ey, ey)
            if abs(cy) < 6.0:
                continue  # keep the street clear
            sx, sy, hgt = rng.uniform(1.0, 6.0), rng.uniform(1.0, 6.0), rng.uniform(1.0, 8.0)
            boxes.append([cx - sx, cy - sy, 0.0, cx + sx, cy + sy, hgt])
        self.boxes = np.array(boxes, dtype=np.float64)
        self.wall = np.array([-ex - 5, -ey - 5, -1.0, ex + 5, ey + 5, wall_height], dtype=np.float64)


class OusterSim:
    def __init__(self, scene, beams=128, cols=1024, fov_deg=22.5, range_min=0.5, range_max=250.0,
                 range_noise=0.02):
        self.scene = scene
        self.beams, self.cols = beams, cols
        alt = np.deg2rad(np.linspace(fov_deg / 2, -fov_deg / 2, beams))
        az = np.linspace(0.0, 2 * np.pi, cols, endpoint=False)
        A, B = np.meshgrid(alt, az, indexing="ij")
        self.dirs = np.stack([np.cos(A) * np.cos(B), np.cos(A) * np.sin(B), np.sin(A)], -1).reshape(-1, 3)
        self.rmin, self.rmax, self.noise = range_min, range_max, range_noise

    def scan(self, T_world_sensor, seed=0):
        """Points in the SENSOR frame (float32), in firing order, misses dropped."""
        rng = np.random.default_rng(seed)
        T = np.asarray(T_world_sensor, dtype=np.float64)
        o = T[:3, 3].astype(np.float32)
        out = []
        chunk = 32768
        bx = self.scene.boxes.astype(np.float32)
        for s in range(0, len(self.dirs), chunk):
            db = self.dirs[s:s + chunk]
            d = (db @ T[:3, :3].T).astype(np.float32)
            t = np.full(len(d), np.inf, dtype=np.float32)
            # ground
            dz = d[:, 2]
            tg = np.where(dz < -1e-9, -o[2] / np.where(dz < -1e-9, dz, -1.0), np.inf)
            t = np.minimum(t, np.where(tg > 0, tg, np.inf))
            inv = (1.0 / np.where(np.abs(d) < 1e-12, 1e-12, d)).astype(np.float32)
            # boxes: slab test per axis (2-D temporaries), nearest entry
            tn = np.full((len(d), len(bx)), -np.inf, dtype=np.float32)
            tf = np.full((len(d), len(bx)), np.inf, dtype=np.float32)
            for a in range(3):
                t1 = (bx[None, :, a] - o[a]) * inv[:, a, None]
                t2 = (bx[None, :, 3 + a] - o[a]) * inv[:, a, None]
                np.maximum(tn, np.minimum(t1, t2), out=tn)
                np.minimum(tf, np.maximum(t1, t2), out=tf)
            hit = (tf >= np.maximum(tn, 0.0)) & (tn > 0.0)
            t = np.minimum(t, np.where(hit, tn, np.inf).min(-1))
            # enclosing walls, seen from inside: exit distance; the open top is a miss
            w = self.scene.wall.astype(np.float32)
            t1 = (w[None, 0:3] - o[None, :]) * inv
            t2 = (w[None, 3:6] - o[None, :]) * inv
            tfar_axis = np.maximum(t1, t2)
            tw = tfar_axis.min(-1)
            top_exit = (np.argmin(tfar_axis, -1) == 2) & (d[:, 2] > 0)
            t = np.minimum(t, np.where(top_exit, np.inf, tw))
            r = t.astype(np.float64) + rng.normal(0.0, self.noise, len(t))
            ok = np.isfinite(t) & (r >= self.rmin) & (r <= self.rmax)
            out.append((db[ok] * r[ok, None]).astype(np.float32))
        return np.concatenate(out)


def voxel_downsample(pts, leaf):
    """First point per voxel (order-preserving), like a coarse pcl::VoxelGrid."""
    key = np.floor(pts.astype(np.float64) / leaf).astype(np.int64)
    key -= key.min(0)
    dims = key.max(0) + 1
    flat = (key[:, 2] * dims[1] + key[:, 1]) * dims[0] + key[:, 0]
    _, first = np.unique(flat, return_index=True)
    return pts[np.sort(first)]


# --------------------------------------------------------------------------- configs
def config_c1(max_points=10000):
    """C1: two 10k-point clouds, 1.0 m voxel."""
    src, tgt, gt, guess = two_planes(seed=1337, max_points=max_points)
    return dict(name="C1 two-plane 10k/10k, 1.0 m", source=src, target=tgt, gt=gt, guess=guess,
                resolution=1.0)


def config_c2(beams=128, cols=1024, seed=42):
    """C2: 128x1024 scan-to-scan, 1.0 m voxel; offset (0.5 m, 0.1 m, 2 deg yaw)."""
    scene = Scene(seed=seed)
    sim = OusterSim(scene, beams=beams, cols=cols)
    Ta = pose_matrix(0.0, 0.0, 2.0, 0.0, 0.0, 0.0)
    Tb = Ta @ pose_matrix(0.5, 0.1, 0.0, 0.0, 0.0, np.deg2rad(2.0))
    tgt = sim.scan(Ta, seed=seed + 1)
    src = sim.scan(Tb, seed=seed + 2)
    gt = np.linalg.inv(Ta) @ Tb
    return dict(name="C2 %dx%d scan-to-scan, 1.0 m" % (beams, cols), source=src, target=tgt, gt=gt,
                guess=np.eye(4), resolution=1.0)


def _cached(name, builder):
    """Generated workloads are cached under $NDT_SYNTH_CACHE (default /tmp/ndt_synth)."""
    import os
    d = os.environ.get("NDT_SYNTH_CACHE", "/tmp/ndt_synth")
    path = os.path.join(d, name + ".npz")
    try:
        z = np.load(path, allow_pickle=False)
        return {k: (z[k] if z[k].ndim else z[k].item()) for k in z.files}
    except Exception:
        pass
    cfg = builder()
    try:
        os.makedirs(d, exist_ok=True)
        tmp = path + ".%d.tmp.npz" % os.getpid()
        np.savez(tmp, **cfg)
        os.replace(tmp, path)
    except Exception:
        pass
    return cfg


def config_c3(n_map=1000000, n_src=200000, seed=7, cols=1024):
    return _cached("c3_v2_%d_%d_%d_%d" % (n_map, n_src, seed, cols),
                   lambda: _config_c3(n_map, n_src, seed, cols))


def _config_c3(n_map=1000000, n_src=200000, seed=7, cols=1024):
    """C3/C4: 200k-point scan into a 1M-point submap, 0.5 m voxel.

    Map = 8 scans (256 beams) along a 40 m track, in the map frame, thinned with a
    0.03 m voxel filter and randomly subsampled to exactly n_map points.  Source = a
    fresh 256-beam scan subsampled (order kept) to n_src points; the initial guess is
    off by (0.3 m, 2 deg).
    """
    scene = Scene(seed=42, extent=(140.0, 90.0), n_boxes=90)
    sim = OusterSim(scene, beams=256, cols=cols)
    rng = np.random.default_rng(seed)
    clouds = []
    for k in range(8):
        Tk = pose_matrix(-20.0 + 40.0 * k / 7.0, 0.3 * np.sin(k), 2.0, 0.0, 0.0, 0.02 * k)
        clouds.append(transform(Tk, sim.scan(Tk, seed=100 + k)))
    m = voxel_downsample(np.concatenate(clouds), 0.03)
    if len(m) < n_map:
        raise RuntimeError("map has only %d points" % len(m))
    m = m[np.sort(rng.choice(len(m), size=n_map, replace=False))]
    Ts = pose_matrix(3.7, -0.4, 2.0, 0.004, -0.006, 0.11)
    s = sim.scan(Ts, seed=11)
    if len(s) < n_src:
        raise RuntimeError("scan has only %d points" % len(s))
    s = s[np.sort(np.random.default_rng(11).choice(len(s), size=n_src, replace=False))]
    guess = Ts @ pose_matrix(0.25, -0.15, 0.06, 0.0, 0.0, np.deg2rad(2.0))
    return dict(name="C3 %dk scan into %dk-pt map, 0.5 m" % (n_src // 1000, n_map // 1000), source=s,
                target=m, gt=Ts, guess=guess, resolution=0.5)


# --------------------------------------------------------------------------- C3-wide
def _terrain(x, y):
    """Gentle hills: a few metres of relief over tens of metres."""
    return 3.0 * np.sin(x / 37.0) * np.cos(y / 53.0) + 1.5 * np.sin((x + y) / 17.0) + 0.01 * x


def _wide_surfaces(rng, n_ground, n_wall, half, boxes):
    """Random points on the terrain and on the vertical faces of `boxes` (cx, cy, sx, sy, h)."""
    gx, gy = rng.uniform(-half, half, n_ground), rng.uniform(-half, half, n_ground)
    ground = np.stack([gx, gy, _terrain(gx, gy)], 1)
    b = boxes[rng.integers(0, len(boxes), n_wall)]
    face = rng.integers(0, 4, n_wall)
    u = rng.uniform(-1.0, 1.0, n_wall)
    wx = np.where(face < 2, b[:, 0] + np.where(face == 0, -1.0, 1.0) * b[:, 2], b[:, 0] + u * b[:, 2])
    wy = np.where(face < 2, b[:, 1] + u * b[:, 3], b[:, 1] + np.where(face == 2, -1.0, 1.0) * b[:, 3])
    wz = _terrain(b[:, 0], b[:, 1]) + rng.uniform(0.0, 1.0, n_wall) * b[:, 4]
    return np.concatenate([ground, np.stack([wx, wy, wz], 1)])


def config_c3_wide(n_map=4000000, n_src=200000, seed=21):
    return _cached("c3wide_v3_%d_%d_%d" % (n_map, n_src, seed), lambda: _config_c3_wide(n_map, n_src, seed))


def _config_c3_wide(n_map, n_src, seed):
    """C3-wide: the C3 shape (200k-point scan into a voxelised map, 0.5 m voxel) on a map whose
    voxel table does NOT fit a cache level that C3's does: open terrain of 260 m x 260 m with 60
    buildings, 4M map points -> ~2.9e5 valid leaves (23 MB of records, 70 MB dense index grid)
    against C3's 2.1e4 (1.7 MB).  The map is in random order (no scan coherence); the source is a
    fresh sample of the same surfaces within 100 m of the sensor, in the sensor frame."""
    rng = np.random.default_rng(seed)
    half = 130.0
    nb = 60
    boxes = np.stack([rng.uniform(-half + 10, half - 10, nb), rng.uniform(-half + 10, half - 10, nb),
                      rng.uniform(2.0, 9.0, nb), rng.uniform(2.0, 9.0, nb), rng.uniform(4.0, 12.0, nb)], 1)
    n_wall = n_map // 5
    m = _wide_surfaces(rng, n_map - n_wall, n_wall, half, boxes)
    m = (m + rng.normal(0.0, 0.02, m.shape)).astype(np.float32)
    m = m[rng.permutation(len(m))]
    z0 = float(_terrain(5.0, -3.0)) + 2.0
    Ts = pose_matrix(5.0, -3.0, z0, 0.01, -0.015, 0.35)
    rs = np.random.default_rng(seed + 1)
    cand = _wide_surfaces(rs, 6 * n_src, 2 * n_src, half, boxes)
    d = np.hypot(cand[:, 0] - 5.0, cand[:, 1] + 3.0)
    cand = cand[d < 100.0]
    if len(cand) < n_src:
        raise RuntimeError("wide source has only %d points" % len(cand))
    cand = cand[np.sort(rs.choice(len(cand), size=n_src, replace=False))]
    cand = cand + rs.normal(0.0, 0.02, cand.shape)
    s = transform(np.linalg.inv(Ts), cand).astype(np.float32)
    guess = Ts @ pose_matrix(0.22, -0.12, 0.05, 0.0, 0.0, np.deg2rad(1.5))
    return dict(name="C3-wide %dk scan into %dk-pt open-terrain map, 0.5 m" % (n_src // 1000, n_map // 1000),
                source=s, target=m, gt=Ts, guess=guess, resolution=0.5)


# --------------------------------------------------------------------------- range images
# The analytic scene of range_image(): a ground plane and two walls, each {x : normal . x = offset} in the world frame.
RANGE_SCENE_PLANES = (((0.0, 0.0, 1.0), 0.0), ((1.0, 0.0, 0.0), 30.0), ((0.0, 1.0, 0.0), -20.0))


def _rodrigues_many(w, u):
    """Exp(u_i w) for a rotation vector w and factors u [m] -> [m, 3, 3]"""
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.broadcast_to(np.eye(3), (len(u), 3, 3)).copy()
    k = w / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    a = np.asarray(u, np.float64) * th
    return np.eye(3) + np.sin(a)[:, None, None] * K + (2.0 * np.sin(0.5 * a) ** 2)[:, None, None] * (K @ K)


def trajectory_poses(knot_t, knot_poses, t):
    """The pose body -> world of the deskew model at the times t [m] (clamped to the knots): the attitude along the
    geodesic between the two knots, the position blended linearly -> (R [m, 3, 3], p [m, 3])."""
    kt, kp = np.asarray(knot_t, np.float64), np.asarray(knot_poses, np.float64)
    t = np.clip(np.asarray(t, np.float64), kt[0], kt[-1])
    R = np.broadcast_to(kp[0][:3, :3], (len(t), 3, 3)).copy()
    p = np.broadcast_to(kp[0][:3, 3], (len(t), 3)).copy()
    if len(kt) == 1:
        return R, p
    seg = np.clip(np.searchsorted(kt, t, side="right") - 1, 0, len(kt) - 2)
    for k in range(len(kt) - 1):
        m = seg == k
        if not m.any():
            continue
        u = (t[m] - kt[k]) / (kt[k + 1] - kt[k])
        R[m] = kp[k][:3, :3] @ _rodrigues_many(so3_log(kp[k][:3, :3].T @ kp[k + 1][:3, :3]), u)
        p[m] = kp[k][:3, 3] + u[:, None] * (kp[k + 1][:3, 3] - kp[k][:3, 3])
    return R, p


def range_image(model, knot_t, knot_poses, col_t, seed=0, no_return=0.05, drop_columns=0, range_max=200.0, range_min=0.3):
    """A seeded lidar range image of RANGE_SCENE_PLANES seen from a sensor that moves along the trajectory (knot_t,
    knot_poses: body -> world, the deskew model) while it scans: column c is taken at col_t[c] (rounded to float32, as
    the image carries it) through the scan model `model` = (x1, y1, z1 [n_cols, n_rows], x2, y2, z2 [n_cols]) -- the ray
    of pixel (c, r) leaves (x2, y2, z2)[c] along (x1, y1, z1)[c, r] in the body frame, the range is the factor of that
    direction as the unprojection applies it.  Ranges are quantised to whole millimetres (0: no surface within
    [range_min, range_max] m), reflectivities are drawn, a share `no_return` of the pixels is zeroed and `drop_columns`
    columns get a NaN time (their ranges stay: the time alone marks them).  Returns a dict: range_mm uint32 and
    reflectivity uint8 [n_cols, n_rows], col_t float32 [n_cols], surface int8 [n_cols, n_rows] (the plane a pixel was
    cast at, -1: none), dropped (the column indices), planes."""
    x1, y1, z1, x2, y2, z2 = (np.asarray(a, np.float32).astype(np.float64) for a in model)
    n_cols, n_rows = x1.shape
    rng = np.random.default_rng(seed)
    t32 = np.asarray(col_t, np.float32).ravel()
    assert len(t32) == n_cols and np.isfinite(t32).all()
    R, p = trajectory_poses(knot_t, knot_poses, t32.astype(np.float64))
    origin = np.einsum("cij,cj->ci", R, np.stack([x2, y2, z2], 1)) + p                 # [n_cols, 3], world
    direction = np.einsum("cij,crj->cri", R, np.stack([x1, y1, z1], 2))                # [n_cols, n_rows, 3]
    best = np.full((n_cols, n_rows), np.inf)
    surface = np.full((n_cols, n_rows), -1, np.int8)
    for s, (normal, offset) in enumerate(RANGE_SCENE_PLANES):
        normal = np.asarray(normal, np.float64)
        den = direction @ normal
        with np.errstate(divide="ignore", invalid="ignore"):
            r = (offset - origin @ normal)[:, None] / den
        hit = np.isfinite(r) & (r >= range_min) & (r <= range_max) & (r < best)
        best[hit] = r[hit]
        surface[hit] = s
    range_mm = np.where(surface >= 0, np.rint(np.where(surface >= 0, best, 0.0) * 1000.0), 0.0).astype(np.uint32)
    lost = rng.uniform(size=(n_cols, n_rows)) < no_return
    range_mm[lost] = 0
    surface[lost | (range_mm == 0)] = -1
    reflectivity = rng.integers(0, 256, (n_cols, n_rows)).astype(np.uint8)
    dropped = np.sort(rng.choice(n_cols, size=int(drop_columns), replace=False)) if drop_columns else np.zeros(0, np.int64)
    t_out = t32.copy()
    t_out[dropped] = np.nan
    return dict(range_mm=range_mm, reflectivity=reflectivity, col_t=t_out, surface=surface, dropped=dropped,
                planes=RANGE_SCENE_PLANES)


def unproject_numpy(model, range_mm, col_t, knot_t=None, knot_poses=None, ref_pose=None):
    """The unprojection (and, with knots, the deskew into ref_pose, None: the last knot) in float64 on the host, a
    reference for tests: [n_cols, n_rows, 3], NaN where a pixel has no return or its column no time."""
    x1, y1, z1, x2, y2, z2 = (np.asarray(a, np.float32).astype(np.float64) for a in model)
    rm = (np.asarray(range_mm, np.uint32).astype(np.float32) * np.float32(0.001)).astype(np.float64)
    pts = np.stack([rm * x1 + x2[:, None], rm * y1 + y2[:, None], rm * z1 + z2[:, None]], 2)
    t = np.asarray(col_t, np.float32).astype(np.float64)
    bad = (np.asarray(range_mm) == 0) | ~np.isfinite(t)[:, None]
    if knot_t is not None:
        ref = np.asarray(knot_poses, np.float64)[-1] if ref_pose is None else np.asarray(ref_pose, np.float64)
        R, p = trajectory_poses(knot_t, knot_poses, np.where(np.isfinite(t), t, 0.0))
        world = np.einsum("cij,crj->cri", R, pts) + p[:, None, :]
        pts = (world - ref[:3, 3]) @ ref[:3, :3]
    pts[bad] = np.nan
    return pts


# --------------------------------------------------------------------------- lidar packets (ndt_packet_* in ndt_hip.h)
PACKET_PROFILE_RNG19, PACKET_PROFILE_LEGACY = 0, 1


def packet_layout(profile, cpp, n_rows):
    """(packet header bytes, block bytes, first pixel offset in a block, packet bytes) of a profile: the table of
    include/ndt_hip.h"""
    legacy = int(profile) == PACKET_PROFILE_LEGACY
    first = 16 if legacy else 12
    block = first + 12 * int(n_rows) + (4 if legacy else 0)
    return (0 if legacy else 32), block, first, (0 if legacy else 64) + int(cpp) * block


def encode_packets(n_cols, n_rows, profile, cpp, range_mm, reflectivity, signal, nir, ts_ns, frame_id, seed=0, garbage=True,
                   order=None, duplicate=(), invalid_status=(), bad_m_id=(), other_frame=(), wrong_type=()):
    """The UDP payloads of one lidar frame from its range image: range_mm (uint32), reflectivity (uint8), signal and nir
    (uint16) [n_cols, n_rows], ts_ns (uint64 [n_cols], the column timestamps).  Packet k carries columns k * cpp ..
    k * cpp + cpp - 1; columns beyond n_cols in the last packet carry m_id = n_cols and an invalid status.  Returns a uint8
    array [n_packets, packet bytes].  Knobs (seeded):
      garbage         random bits where the format has none to read: the high bits of d0 (19-31 RNG19, 20-31 LEGACY), bytes
                      5, 10 and 11 of a pixel, the packet header and footer beyond type and frame id, the spare header bytes
      order           which packets go out and in which order (indices, default all in order): drops and reorders
      duplicate       packets emitted once more at the END with other pixel contents (the later arrival must win)
      invalid_status  columns (m_id) sent with an invalid status
      bad_m_id        columns sent with m_id = n_cols
      other_frame     LEGACY: columns whose own frame id field is frame_id + 1
      wrong_type      RNG19: packets (indices before `order`) sent with packet type 2"""
    n_cols, n_rows, cpp = int(n_cols), int(n_rows), int(cpp)
    legacy = int(profile) == PACKET_PROFILE_LEGACY
    header, block, first, size = packet_layout(profile, cpp, n_rows)
    rng = np.random.default_rng(seed)
    r = np.asarray(range_mm, np.uint32).reshape(n_cols, n_rows)
    mask = np.uint32(0x000FFFFF if legacy else 0x0007FFFF)
    assert np.all(r <= mask)
    d = np.zeros((n_cols, n_rows, 3), np.uint32)
    d[:, :, 0] = r
    d[:, :, 1] = np.asarray(reflectivity, np.uint8).reshape(n_cols, n_rows).astype(np.uint32) | \
        (np.asarray(signal, np.uint16).reshape(n_cols, n_rows).astype(np.uint32) << np.uint32(16))
    d[:, :, 2] = np.asarray(nir, np.uint16).reshape(n_cols, n_rows).astype(np.uint32)
    ts = np.asarray(ts_ns, np.uint64).ravel()
    assert len(ts) == n_cols
    n_packets = (n_cols + cpp - 1) // cpp

    def junk(shape, keep_mask):
        g = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32) if garbage else np.zeros(shape, np.uint32)
        return g & ~np.uint32(keep_mask)

    def build(k, pixels):
        p = (rng.integers(0, 256, size).astype(np.uint8) if garbage else np.zeros(size, np.uint8))
        if not legacy:
            p[0:2] = np.frombuffer(np.uint16(2 if k in wrong_type else 1).tobytes(), np.uint8)
            p[2:4] = np.frombuffer(np.uint16(frame_id).tobytes(), np.uint8)
        for c in range(cpp):
            m = k * cpp + c
            b = header + c * block
            live = m < n_cols
            m_field = m if live and m not in bad_m_id else n_cols
            p[b:b + 8] = np.frombuffer(np.uint64(ts[m] if live else 0).tobytes(), np.uint8)
            p[b + 8:b + 10] = np.frombuffer(np.uint16(m_field).tobytes(), np.uint8)
            ok = live and m not in invalid_status
            if legacy:
                p[b + 10:b + 12] = np.frombuffer(np.uint16((frame_id + 1) & 0xFFFF if m in other_frame else frame_id).tobytes(), np.uint8)
                status = 0xFFFFFFFF if ok else int(rng.integers(0, 0xFFFFFFFF))
                p[b + 16 + 12 * n_rows:b + 20 + 12 * n_rows] = np.frombuffer(np.uint32(status).tobytes(), np.uint8)
            else:
                p[b + 10] = (p[b + 10] & 0xFE) | (1 if ok else 0)
            if live:
                px = pixels[m].copy()
                px[:, 0] |= junk(n_rows, mask)
                px[:, 1] |= junk(n_rows, 0xFFFF00FF)                 # byte 5
                px[:, 2] |= junk(n_rows, 0x0000FFFF)                 # bytes 10 and 11
                p[b + first:b + first + 12 * n_rows] = np.frombuffer(px.astype("<u4").tobytes(), np.uint8)
        return p

    natural = list(range(n_packets)) if order is None else [int(k) for k in order]
    out = [build(k, d) for k in natural]
    for k in duplicate:
        other = d.copy()
        other[:, :, 0] = rng.integers(1, int(mask) + 1, (n_cols, n_rows)).astype(np.uint32)
        other[:, :, 1] = rng.integers(0, 2 ** 32, (n_cols, n_rows), dtype=np.uint64).astype(np.uint32) & np.uint32(0xFFFF00FF)
        other[:, :, 2] = rng.integers(0, 2 ** 16, (n_cols, n_rows)).astype(np.uint32)
        out.append(build(int(k), other))
    return np.stack(out) if out else np.zeros((0, size), np.uint8)
