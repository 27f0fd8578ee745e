"""The voxel-grid build on each of its pipelines, at the limits of the two-launch build, and across rebuilds of one
handle, against the CPU oracle.

Pipelines (ndt_target.hip; which one runs is decided in ndt_handoff.hip build_begin / build_enqueue / build_collect):
  A  first build of a handle, fused digit passes          B  first build, classic digit passes (fused_sort=0)
  C  steady state, sort-based (bucket_build=0)            D  steady state, two launches (k_bucket_pass + k_bucket_leaves)
  E  D with the partition's tile forced to 1024 / 2048 / 4096 / 8192 points
A first build is always sort-based, so only a second build on a handle reaches D and E.  buildCounters() proves which
pipeline ran: `HandleModel` restates the host's decision (grid capacity, back-off after a decline), and `bucket_stats`
restates k_bucket_pass's hashing of voxels into 256 buckets, so each build's counter deltas are predicted, not read back.

The limits of the two-launch build, per bucket (one bucket = one 1024-thread block of k_bucket_leaves):
  <= 256 distinct cells: the leaf list comes straight out of the one digit pass; 257..3584: two digit passes and the
  general run search; > 3584 (or a full LDS hash table): declined late; > 8192 points: declined; <= 2730 leaves;
  voxels above LEAF_HEAD = 64 points are finished by the whole wave.  Non-finite points ride in bucket 0 as one
  sentinel "cell" that is never a leaf; voxel indices of 2^23 and beyond are declined before anything is written.

After every build: grid geometry and leaves against the oracle (cell and count exact, mean 1e-12, cov / icov / evals
within test_gpu_random's cancellation-aware bound), the same bits on every pipeline, and one evaluation per
neighbourhood (DIRECT7, KDTREE) against the oracle's f64 evaluation (pair_mode=2) -- the only check that sees the dense
cell -> leaf index and the centroid table, where a cell left over from the previous build would show."""
import numpy as np
import pytest

from test_gpu_random import cov_loss, make_cloud

M32 = 0xFFFFFFFF
BK_MAXP, BK_MAX_DISTINCT, BK_MAX_LEAVES, BK_COORD_LIMIT = 8192, 3584, 2730, 2 ** 23
FITS = 256 * 8192 * 5 // 8   # bucket_build_fits: 1 310 720 points
TILES = (1024, 2048, 4096, 8192)
LEAF_FIELDS = ("cell", "count", "mean", "cov", "icov", "evals", "evecs")


# ---------------------------------------------------------------------------------------------------------------------
# restatement of the two-launch build's bucketing (ndt_target.hip bucket_of, k_bucket_pass, k_bucket_leaves)
# ---------------------------------------------------------------------------------------------------------------------
def cell_floor(p, res):
    """floor(p * inv_leaf) in f32, inv_leaf = 1.0f / resolution, as every build kernel forms it."""
    inv = np.float32(1.0) / np.float32(res)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor(np.asarray(p, np.float32) * inv)


def bucket_of(cells):
    """ndt_target.hip bucket_of() in uint32 arithmetic: cells are integral (floor'd) values; negative ones wrap as
    (uint32_t)__float2int_rz does."""
    ijk = [np.asarray(cells)[:, a].astype(np.int64) & M32 for a in range(3)]
    h = ((ijk[0] * 0x9E3779B1) & M32) ^ ((ijk[1] * 0x85EBCA77) & M32) ^ ((ijk[2] * 0xC2B2AE3D) & M32)
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & M32
    h ^= h >> 12
    h = (h * 0x297A2D39) & M32
    h ^= h >> 15
    return h >> 24


def bucket_stats(p, res, min_pts):
    """Per bucket: points (non-finite ones in bucket 0), distinct keys (bucket 0's sentinel included) and leaves
    (voxels of >= min_pts points); and whether the two-launch build declines the cloud."""
    p = np.asarray(p, np.float32)
    fin = np.isfinite(p).all(axis=1)
    nbad = int((~fin).sum())
    c = cell_floor(p[fin], res).astype(np.int64)
    if len(c):   # one int64 key per cell (np.unique over rows is slow)
        lo, span = c.min(axis=0), c.max(axis=0) - c.min(axis=0) + 1
        key = ((c[:, 0] - lo[0]) * span[1] + (c[:, 1] - lo[1])) * span[2] + (c[:, 2] - lo[2])
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        cells = c[first]
    else:
        cells, inv = c, np.zeros(0, np.int64)
    per_cell = np.bincount(inv.ravel(), minlength=len(cells))
    b = bucket_of(cells) if len(cells) else np.zeros(0, np.int64)
    points = np.bincount(b, weights=per_cell, minlength=256).astype(np.int64)
    distinct = np.bincount(b, minlength=256)
    leaves = np.bincount(b, weights=per_cell >= max(3, min_pts), minlength=256).astype(np.int64)
    points[0] += nbad
    distinct[0] += nbad > 0
    far = bool(len(cells)) and bool((np.abs(cells) >= BK_COORD_LIMIT).any())
    declined = bool((points > BK_MAXP).any() or (distinct > BK_MAX_DISTINCT).any() or far)
    return dict(points=points, distinct=distinct, leaves=leaves, declined=declined, far=far,
                max_voxel=int(per_cell.max()) if len(cells) else 0)


# ---------------------------------------------------------------------------------------------------------------------
# generators: exact counts in one chosen bucket, every other point in buckets far below the limits
# ---------------------------------------------------------------------------------------------------------------------
def cells_in_bucket(b, k, lo=(0, 0, 0), shape=(128, 128, 80)):
    """The first k integer cells of the box lo + [0, shape) that hash to bucket b."""
    c = np.indices(shape).reshape(3, -1).T.astype(np.int64) + np.asarray(lo, np.int64)
    c = c[bucket_of(c) == b]
    assert len(c) >= k, (b, k, len(c))
    return c[:k]


def fill(rng, cells, counts, res):
    """counts[i] points (counts cycled) strictly inside cell i (res a power of two: the f32 floor gives the cell back exactly)."""
    counts = np.resize(np.asarray(counts), len(cells))   # (a short list repeats)
    c = np.repeat(np.asarray(cells, np.float64), counts, axis=0)
    return ((c + rng.uniform(0.05, 0.95, c.shape)) * res).astype(np.float32)


def background(rng, avoid, res, n_cells=300):
    """Ordinary voxels (3..12 points) in the negative octant, in no bucket listed in `avoid`."""
    c = np.indices((24, 24, 8)).reshape(3, -1).T.astype(np.int64) - np.array([40, 40, 12])
    c = c[~np.isin(bucket_of(c), list(avoid))]
    c = c[rng.choice(len(c), n_cells, replace=False)]
    return fill(rng, c, rng.integers(3, 13, n_cells), res)


def nonfinite(k):
    rows = np.array([[np.nan, np.nan, np.nan], [np.inf, 0.0, 1.0], [0.5, -np.inf, np.nan]], np.float32)
    return rows[np.arange(k) % 3]


def limit_cloud(seed, b, cells, counts, nan=0, res=1.0):
    """Bucket b holds `cells` with `counts` points each and `nan` non-finite
    points; the rest of the cloud is background in other buckets.  Shuffled: a bucket's points arrive in input order
    from many tiles."""
    rng = np.random.default_rng(seed)
    parts = [fill(rng, cells, counts, res), background(rng, {b}, res), nonfinite(nan)]
    p = np.concatenate(parts)
    return p[rng.permutation(len(p))]


def _crowded(seed, n_small):
    """Voxels of 63 / 64 / 65 / 127 / 128 / 129 / 4096 points around LEAF_HEAD, all in bucket 9 (several crowded
    leaves in one wave), among n_small ordinary voxels of the same bucket."""
    cells = cells_in_bucket(9, 7 + n_small)
    sizes = [63, 64, 65, 127, 128, 129, 4096] + [4, 6, 9, 2] * (n_small // 4)
    return limit_cloud(seed, 9, cells, sizes)


def _coords(seed, x0, n=20000):
    """A slab at voxel index x0 .. x0 + 50 in x (resolution 1): below 2^23 the two-launch build takes it, at and
    beyond 2^23 it declines before writing anything."""
    rng = np.random.default_rng(seed)
    p = np.stack([x0 + rng.uniform(0.0, 50.0, n), rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)], axis=1)
    return p.astype(np.float32)


def _faces(seed, n=30000):
    """Resolution 0.5: a third of the coordinates lie exactly on voxel faces, some are -0.0 / +0.0; all octants."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-6.0, 6.0, (n, 3))
    k = rng.integers(0, 3, n)
    on = rng.random(n) < 0.33
    p[on, k[on]] = np.round(p[on, k[on]] * 2.0) / 2.0
    z = rng.random(n) < 0.02
    p[z, 0] = -0.0
    p[z, 1] = 0.0
    p = p.astype(np.float32)
    p[z, 2] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    return p


def _uniform(seed, n, half=20.0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-half, half, (n, 3)).astype(np.float32)
    p[rng.integers(0, n, 7)] = np.nan
    return p


def _random(seed, kind, n, offset, bad):
    rng = np.random.default_rng(seed)
    p = make_cloud(rng, kind, n, np.asarray(offset, np.float64) * np.array([1.0, -0.5, 0.1]))
    if bad:
        p[rng.integers(0, n, max(1, n // 50))] = np.nan
    return p


# name -> (factory, resolution, min_pts, what the restatement must show for it)
CORPUS = {}
for _i, (_kind, _n, _res, _mp, _off, _bad) in enumerate([
        ("blobs", 20000, 1.0, 6, 0.0, False), ("planes", 30000, 0.3, 6, -37.5, True), ("lines", 5000, 1.7, 10, 1500.0, False),
        ("dupes", 40000, 1.0, 3, 0.0, True), ("box", 60000, 1.7, 6, -37.5, False), ("blobs", 50000, 0.3, 10, 1500.0, True),
        ("planes", 8000, 1.0, 1, 0.0, False), ("lines", 60000, 0.3, 3, -37.5, True), ("dupes", 12000, 1.7, 6, 1500.0, False),
        ("box", 25000, 1.0, 10, 0.0, True), ("blobs", 7000, 1.7, 3, -37.5, False), ("planes", 45000, 1.7, 10, 1500.0, True),
        ("lines", 15000, 1.0, 6, 0.0, True), ("dupes", 5000, 0.3, 1, -37.5, False), ("box", 35000, 0.3, 6, 1500.0, True),
        ("blobs", 60000, 1.0, 1, -37.5, True), ("planes", 20000, 1.7, 3, 0.0, False), ("lines", 9000, 0.3, 6, 1500.0, False),
        ("dupes", 55000, 1.0, 10, -37.5, True), ("box", 10000, 1.0, 3, 1500.0, False)]):
    CORPUS["%s%d-n%d-r%g-m%d%s%s" % (_kind, _i, _n, _res, _mp, "-o%g" % _off if _off else "", "-nan" if _bad else "")] = (
        lambda s=_i, k=_kind, n=_n, o=_off, b=_bad: _random(3000 + s, k, n, o, b), _res, _mp, {})
LIMITS = {
    # distinct cells in one bucket: one digit pass / two passes; the hash table's limit
    "cells256": (lambda: limit_cloud(1, 17, cells_in_bucket(17, 256), [6, 2, 7, 3]), 1.0, 6, dict(b=17, distinct=256)),
    "cells257": (lambda: limit_cloud(2, 17, cells_in_bucket(17, 257), [6, 2, 7, 3]), 1.0, 6, dict(b=17, distinct=257)),
    "cells3584": (lambda: limit_cloud(3, 40, cells_in_bucket(40, 3584), [2, 3, 1, 2]), 1.0, 3, dict(b=40, distinct=3584)),
    "cells3585": (lambda: limit_cloud(4, 40, cells_in_bucket(40, 3585), [2, 3, 1, 2]), 1.0, 3,
                  dict(b=40, distinct=3585, declined=True)),
    # points in one bucket
    "points8192": (lambda: limit_cloud(5, 77, cells_in_bucket(77, 1024), 8), 1.0, 6, dict(b=77, points=8192)),
    "points8193": (lambda: limit_cloud(6, 77, cells_in_bucket(77, 1025), [8] * 1024 + [1]), 1.0, 6,
                   dict(b=77, points=8193, declined=True)),
    # the most leaves a bucket block can hold (min_pts 1 is clamped to 3)
    "leaves2730": (lambda: limit_cloud(7, 130, cells_in_bucket(130, 2730), 3), 1.0, 1, dict(b=130, leaves=BK_MAX_LEAVES, points=8190)),
    # one voxel filling a bucket block, and one beyond it
    "voxel8192": (lambda: limit_cloud(8, 201, cells_in_bucket(201, 1), 8192), 1.0, 6, dict(b=201, points=8192, max_voxel=8192)),
    "voxel8193": (lambda: limit_cloud(9, 201, cells_in_bucket(201, 1), 8193), 1.0, 6,
                  dict(b=201, points=8193, max_voxel=8193, declined=True)),
    "crowded": (lambda: _crowded(10, 200), 1.0, 6, dict(b=9, distinct=207, leaves=107, points=5722, max_voxel=4096)),
    "crowded-general": (lambda: _crowded(26, 300), 1.0, 6, dict(b=9, distinct=307, leaves=157, max_voxel=4096)),
    # bucket 0 with non-finite points: the sentinel run below / at min_pts (one digit pass and general run search),
    # bucket 0 filled to 8192 / 8193 points by them, and 3583 / 3584 real cells next to the sentinel
    "nan-below": (lambda: limit_cloud(11, 0, cells_in_bucket(0, 100), 6, nan=5), 1.0, 6, dict(b=0, distinct=101, points=605)),
    "nan-exact": (lambda: limit_cloud(12, 0, cells_in_bucket(0, 100), 6, nan=6), 1.0, 6, dict(b=0, distinct=101, points=606)),
    "nan-exact-general": (lambda: limit_cloud(13, 0, cells_in_bucket(0, 300), 6, nan=6), 1.0, 6,
                          dict(b=0, distinct=301, points=1806)),
    "nan-8192": (lambda: limit_cloud(14, 0, cells_in_bucket(0, 300), 6, nan=6392), 1.0, 6, dict(b=0, distinct=301, points=8192)),
    "nan-8193": (lambda: limit_cloud(15, 0, cells_in_bucket(0, 300), 6, nan=6393), 1.0, 6,
                 dict(b=0, distinct=301, points=8193, declined=True)),
    "b0-3583": (lambda: limit_cloud(16, 0, cells_in_bucket(0, 3583), 2, nan=3), 1.0, 3, dict(b=0, distinct=3584)),
    "b0-3584": (lambda: limit_cloud(17, 0, cells_in_bucket(0, 3584), 2, nan=3), 1.0, 3, dict(b=0, distinct=3585, declined=True)),
    # voxel indices at 2^23 (BK_COORD_LIMIT), both signs
    "coord-below": (lambda: _coords(18, BK_COORD_LIMIT - 60), 1.0, 6, dict(far=False)),
    "coord-above": (lambda: _coords(19, BK_COORD_LIMIT), 1.0, 6, dict(far=True, declined=True, thin=True)),
    "coord-neg-below": (lambda: _coords(20, -BK_COORD_LIMIT + 1), 1.0, 6, dict(far=False)),
    "coord-neg-above": (lambda: _coords(21, -BK_COORD_LIMIT - 10), 1.0, 6, dict(far=True, declined=True, thin=True)),
    "faces": (lambda: _faces(22), 0.5, 6, {}),
    # sizes: n = 1, 2, 7, a ragged last tile, the tile-size switches of bucket_rounds_for and the fits limit
    "n1": (lambda: np.array([[0.25, 0.5, 0.75]], np.float32), 1.0, 3, {}),
    "n2": (lambda: np.array([[0.25, 0.5, 0.75], [0.3, 0.2, 0.1]], np.float32), 1.0, 3, {}),
    "n7": (lambda: np.random.default_rng(24).uniform(0.0, 0.99, (7, 3)).astype(np.float32), 1.0, 3, {}),
    "ragged20481": (lambda: _random(25, "blobs", 20481, 0.0, True), 0.5, 6, {}),
}
for _n in (524288, 524289, 1048576, 1048577, 1310720, 1310721):
    LIMITS["n%d" % _n] = (lambda n=_n: _uniform(_n, n), 1.0, 6, {})
CORPUS.update(LIMITS)

# clouds of the rebuild sequences (below), not run through every pipeline on their own
SEQ_CLOUDS = {
    "s-blobs": (lambda: _random(4001, "blobs", 20000, 0.0, False), 1.0, 6, {}),
    "s-box-wide": (lambda: (np.random.default_rng(4002).uniform(-30, 30, (60000, 3)) * [1, 1, 0.07]).astype(np.float32), 1.0, 6, {}),
    "s-small": (lambda: _random(4003, "planes", 7000, 0.0, True), 1.0, 6, {}),
    "s-neg": (lambda: _random(4001, "blobs", 20000, -300.0, False), 1.0, 6, {}),
    "s-lines": (lambda: _random(4004, "lines", 50000, -37.5, True), 1.0, 6, {}),
}
_param_corpus = list(CORPUS)
CORPUS.update(SEQ_CLOUDS)

_clouds = {}


def cloud(name):
    if name not in _clouds:
        _clouds[name] = CORPUS[name][0]()
    return _clouds[name]


def test_generators_place_the_intended_counts():
    """CPU: the limit clouds hold the per-bucket counts they were built for (the GPU tests then confirm, through the
    build counters, that the two-launch build sees the same buckets), and every other bucket stays far below them."""
    for name, (_, res, min_pts, want) in LIMITS.items():
        st = bucket_stats(cloud(name), res, min_pts)
        b = want.get("b")
        if b is None:   # sizes, coordinates, faces: ordinary buckets
            assert st["points"].max() < 7000 and st["distinct"].max() < 400, name
        else:
            for k in ("distinct", "points", "leaves"):
                if k in want:
                    assert st[k][b] == want[k], (name, k, st[k][b])
            others = np.arange(256) != b
            assert st["points"][others].max() < 100 and st["distinct"][others].max() < 20, name
        assert st["declined"] == want.get("declined", False), name
        assert st["far"] == want.get("far", False), name
        if "max_voxel" in want:
            assert st["max_voxel"] == want["max_voxel"], name
    for name in SEQ_CLOUDS:
        st = bucket_stats(cloud(name), CORPUS[name][1], CORPUS[name][2])
        assert not st["declined"] and st["points"].max() < 2000, name
    # negative indices wrap as (uint32_t)__float2int_rz does
    assert bucket_of(np.array([[-1, 0, 0]]))[0] == bucket_of(np.array([[M32, 0, 0]]))[0]


# ---------------------------------------------------------------------------------------------------------------------
# the host's choice of pipeline (ndt_handoff.hip), restated
# ---------------------------------------------------------------------------------------------------------------------
class HandleModel:
    """Predicts each build's buildCounters() delta on one handle: a steady-state ("optimistic") build needs the
    previous build to have gone through and the leaf table to hold this cloud's worst case; it takes two launches
    when the two-launch build is on, the cloud fits and no back-off is pending, unless the grid is too small (BG_CAPACITY:
    repeated waiting for the geometry, not counted) or a bucket is beyond a block (declined, counted, back-off 8, 16, ...
    64 builds).  Buffers grow to n + n / 8 + 64 (DevBuf::ensure)."""

    def __init__(self, bucket_build=True):
        self.bucket_build = bucket_build
        self.c2l = self.stats = 0
        self.clean = False
        self.backoff = self.skip = 0

    def build(self, n, ncells, min_pts, declined):
        grow = lambda need, cap: cap if need <= cap else need + need // 8 + 64   # noqa: E731
        max_leaves = n // max(3, min_pts) + 1
        optimistic = self.clean and max_leaves <= self.stats
        ok = self.bucket_build and 0 < n <= FITS
        if ok and self.skip > 0:
            self.skip -= 1
            ok = False
        delta = (0, 0, 0)
        if ok and optimistic and ncells <= self.c2l:
            if declined:
                delta = (0, 1, 0)
                self.backoff = min(64, max(8, 2 * self.backoff))
                self.skip = self.backoff
            else:
                delta = (0, 0, 1)
                self.backoff = 0
        self.c2l, self.stats, self.clean = grow(ncells, self.c2l), grow(max_leaves, self.stats), True
        return delta


# ---------------------------------------------------------------------------------------------------------------------
# oracle side, cached per (cloud, resolution, min_pts)
# ---------------------------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self, O, S, name, res, min_pts):
        p = cloud(name)
        self.name, self.n, self.res, self.min_pts = name, len(p), res, min_pts
        kw = dict(resolution=res, step_size=0.1, trans_epsilon=1e-4, max_iterations=5, min_points_per_voxel=min_pts)
        self.kw = kw
        self.grid = O.Grid(p, O.default_params(num_threads=8, **kw))
        self.L = self.grid.export()
        self.ncells = int(np.prod(self.grid.div_b))
        self.declined = bucket_stats(p, res, min_pts)["declined"]
        # Beyond 2^23 voxels a voxel is thinner than an f32 ulp: its points share one x, its covariance is cancellation
        # noise (|mean| / spread ~ 2^23: all digits lost), and which voxels pass the eigenvalue checks is noise too, in
        # the oracle as in the kernels.  Those clouds are checked for membership (each leaf's count against the voxel
        # populations restated here) and bit for bit across the pipelines, not for statistics.
        self.thin = CORPUS[name][3].get("thin", False)
        if self.thin:
            f = cell_floor(p[np.isfinite(p).all(axis=1)], res).astype(np.int64) - self.grid.min_b
            d = self.grid.div_b.astype(np.int64)
            self.population = np.bincount(f[:, 0] + f[:, 1] * d[0] + f[:, 2] * d[0] * d[1], minlength=self.ncells)
        self.loss = cov_loss(self.L) if len(self.L["cell"]) else np.zeros(0)
        self.amp = float(self.loss.max()) if len(self.loss) else 0.0
        self.valid = bool((self.L["count"] > 0).any())
        # a source of <= 50 k points near the target: the target seen from a slightly different pose, plus outliers
        rng = np.random.default_rng(len(p) + int(res * 1000) + min_pts)
        fin = p[np.isfinite(p).all(axis=1)]
        far = len(fin) and np.abs(fin).max() > 1.0e4   # (far from the origin: translations only, exact in f32)
        rot = np.zeros(3) if far else rng.normal(0, 0.01, 3)
        dT = S.pose_matrix(*(rng.normal(0, 0.05 * res, 3)), *rot)
        take = fin[rng.choice(len(fin), min(len(fin), 50000), replace=False)] if len(fin) else fin
        src = S.transform(np.linalg.inv(dT), take.astype(np.float64)).astype(np.float32)
        ctr = fin.mean(axis=0) if len(fin) else np.zeros(3)
        self.src = np.concatenate([src, (rng.uniform(-30, 30, (5, 3)) + ctr).astype(np.float32)])
        p0 = O.matrix_to_pose(dT)
        step = rng.normal(0, 0.02 * res, 6)
        if far:
            step[3:] = 0.0
        self.poses = np.stack([p0, p0 + step])
        self.derivs = {}
        if self.valid:
            for m in (O.DIRECT7, O.KDTREE):
                prm = O.default_params(num_threads=8, search_method=m, pair_mode=2, **kw)
                self.derivs[m] = [self.grid.derivatives(self.src, q, params=prm) for q in self.poses]


@pytest.fixture(scope="module")
def refs(O, S):
    cache = {}

    def get(name, res=None, min_pts=None):
        res = CORPUS[name][1] if res is None else res
        min_pts = CORPUS[name][2] if min_pts is None else min_pts
        k = (name, res, min_pts)
        if k not in cache:
            cache[k] = Ref(O, S, name, res, min_pts)
        return cache[k]
    return get


def check_grid(pkg, O, ndt, ref, what):
    """Geometry, leaves and one evaluation per neighbourhood of the handle's current grid against the oracle."""
    gi = ndt.getGridInfo()
    assert np.array_equal(gi["min_b"], ref.grid.min_b) and np.array_equal(gi["div_b"], ref.grid.div_b), what
    L, OL = ndt.getLeaves(), ref.L
    if ref.thin:
        assert len(L["cell"]) and (np.abs(L["count"]) == ref.population[L["cell"]]).all(), what
        assert (np.abs(L["count"]) >= max(3, ref.min_pts)).all(), what
        return L
    assert gi["n_leaves"] == ref.grid.n_leaves, (what, gi["n_leaves"], ref.grid.n_leaves)
    assert np.array_equal(L["cell"], OL["cell"]), what
    assert np.array_equal(L["count"], OL["count"]), what   # (rejected leaves carry a negative count)
    if len(OL["cell"]):
        np.testing.assert_allclose(L["mean"], OL["mean"], rtol=1e-12, atol=0, err_msg=str(what))
        for k, f in (("cov", 1.0), ("icov", 100.0), ("evals", 100.0)):
            ax = (1, 2) if OL[k].ndim == 3 else 1
            err = np.abs(L[k] - OL[k]).max(axis=ax)
            assert (err <= f * ref.loss * np.abs(OL[k]).max(axis=ax)).all(), (what, k, err.max())
    ndt.setInputSource(ref.src)
    if not ref.valid:   # no voxel passed the eigenvalue checks: a loud refusal
        with pytest.raises(pkg.NdtError) as ei:
            ndt.evalDerivatives(ref.poses[0])
        assert ei.value.code == -4, what
        return L
    tol = 1e-9 + 30 * ref.amp
    for method, om in ((pkg.DIRECT7, O.DIRECT7), (pkg.KDTREE, O.KDTREE)):
        ndt.setParams(search_method=method)
        for e, x in zip(ndt.evalDerivatives(ref.poses), ref.derivs[om]):
            w = (what, method)
            assert e["n_pairs"] == x["n_pairs"] and e["n_with_neighbors"] == x["n_with_neighbors"], w
            assert abs(e["score"] - x["score"]) <= tol * abs(x["score"]) + 1e-9, w
            assert abs(e["nvtl_sum"] - x["nvtl_sum"]) <= tol * abs(x["nvtl_sum"]) + 1e-9, w
            assert np.linalg.norm(e["gradient"] - x["gradient"]) <= tol * np.linalg.norm(x["gradient"]) + 1e-9, w
            assert np.linalg.norm(e["hessian"] - x["hessian"]) <= tol * np.linalg.norm(x["hessian"]) + 1e-9, w
    ndt.setParams(search_method=pkg.DIRECT7)
    return L


def same_bits(a, b, what):
    for f in LEAF_FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f)


def counters(ndt):
    return np.array(ndt.buildCounters())


class Tuned:
    """Process-global tuning changed for a block, restored on the way out."""

    def __init__(self, pkg, **fields):
        self.pkg, self.fields = pkg, fields

    def __enter__(self):
        self.before = self.pkg.get_tuning()
        self.pkg.set_tuning(**self.fields)
        return self

    def __exit__(self, *exc):
        self.pkg.set_tuning(**self.before)


def new_ndt(pkg, ref, **kw):
    n, info = pkg.backend_info()
    assert n > 0, "GPU test on a box without a HIP device: " + info
    return pkg.NormalDistributionsTransform(device_id=0, **dict(ref.kw, **kw))


def paths_for(n):
    out = [("A", {}, 1), ("B", dict(fused_sort=0), 1), ("C", dict(bucket_build=0), 2), ("D", {}, 2)]
    out += [("E%d" % t, dict(bucket_tile=t), 2) for t in TILES if 0 < n <= 256 * t and n <= FITS]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", _param_corpus)
def test_every_pipeline_builds_the_oracle_grid(pkg, O, refs, name):
    ref = refs(name)
    p = cloud(name)
    first = None
    for path, tune, builds in paths_for(len(p)):
        with Tuned(pkg, **tune):
            ndt = new_ndt(pkg, ref)
            model = HandleModel(bucket_build=pkg.get_tuning()["bucket_build"] != 0)
            for rep in range(builds):
                c0 = counters(ndt)
                ndt.setInputTarget(p)
                ndt.getGridInfo()   # (waits for a deferred build)
                delta = tuple(counters(ndt) - c0)
                want = model.build(len(p), ref.ncells, ref.min_pts, ref.declined)
                assert delta == want, (name, path, rep, delta, want)
                L = check_grid(pkg, O, ndt, ref, (name, path, rep))
                if first is None:
                    first = L
                else:
                    same_bits(L, first, (name, path, rep))
            ndt.close()


# ---------------------------------------------------------------------------------------------------------------------
# rebuild sequences on one handle
# ---------------------------------------------------------------------------------------------------------------------


def run_sequence(pkg, O, refs, ndt, steps, model, load=None):
    """steps: (cloud name, resolution, min_pts, how) -- how: "target" (setInputTarget), "res" (setResolution),
    "minpts" (setMinPointPerVoxel) or a callable that loads the cloud.  Checks every step against the oracle, its
    counter delta against the model, and its bits against a fresh handle's first build."""
    n_two = 0
    for i, (name, res, min_pts, how) in enumerate(steps):
        ref = refs(name, res, min_pts)
        c0 = counters(ndt)
        if how == "res":
            ndt.setResolution(res)
        elif how == "minpts":
            ndt.setMinPointPerVoxel(min_pts)
        elif how == "target":
            ndt.setInputTarget(cloud(name))
        else:
            how(cloud(name))
        ndt.getGridInfo()   # (waits for a deferred build)
        delta = tuple(counters(ndt) - c0)
        want = model.build(ref.n, ref.ncells, min_pts, ref.declined)
        assert delta == want, (i, name, how, delta, want)
        n_two += delta[2]
        L = check_grid(pkg, O, ndt, ref, (i, name, how))
        fresh = new_ndt(pkg, ref)
        fresh.setInputTarget(cloud(name))
        same_bits(L, fresh.getLeaves(), (i, name, how))
        fresh.close()
    return n_two


@pytest.mark.gpu
def test_rebuilds_grow_shrink_and_move(pkg, O, refs):
    """Clouds alternating in size, extent and sign of coordinates; the wide box outgrows the index grid (BG_CAPACITY:
    the build is repeated waiting for the geometry), the ones after it fit again."""
    seq = ["s-blobs", "s-blobs", "s-box-wide", "s-small", "s-neg", "s-lines", "s-blobs", "s-box-wide", "s-neg", "s-small"]
    ndt = new_ndt(pkg, refs("s-blobs"))
    model = HandleModel()
    n_two = run_sequence(pkg, O, refs, ndt, [(s, 1.0, 6, "target") for s in seq], model)
    assert n_two >= 6, n_two
    ndt.close()


@pytest.mark.gpu
def test_rebuilds_through_a_late_decline_and_the_back_off(pkg, O, refs):
    """A cloud declined late (one bucket of 3585 distinct cells, after the other buckets have published leaves; the
    host clears the whole grid), then ordinary clouds: sort-based for the next 8 builds, then two launches again; a
    second decline backs off again."""
    # (cells3584 first: its grid is large enough that cells3585 is not refused for capacity before it is declined)
    seq = ["cells3584", "cells3584", "cells3585"] + ["s-small", "s-blobs"] * 5 + ["points8193", "s-neg", "s-blobs"]
    steps = [(s, 1.0, 3, "target") for s in seq]   # (the handle's min_pts: cells3584's)
    ndt = new_ndt(pkg, refs("cells3584"))
    n_two = run_sequence(pkg, O, refs, ndt, steps, HandleModel())
    bc = ndt.buildCounters()
    assert bc[1] == 2 and n_two == bc[2] >= 3, bc
    ndt.close()


@pytest.mark.gpu
def test_rebuilds_across_parameter_changes(pkg, O, refs):
    """setResolution / setMinPointPerVoxel re-voxelise the loaded target on the same handle (a rebuild through the same
    pipelines), interleaved with new targets."""
    steps = [("s-blobs", 1.0, 6, "target"), ("s-blobs", 1.0, 6, "target"), ("s-blobs", 0.5, 6, "res"),
             ("s-blobs", 0.5, 3, "minpts"), ("s-lines", 0.5, 3, "target"), ("s-lines", 1.7, 3, "res"),
             ("s-lines", 1.7, 1, "minpts"), ("s-small", 1.7, 1, "target"), ("s-small", 1.0, 1, "res"),
             ("s-small", 1.0, 10, "minpts"), ("s-neg", 1.0, 10, "target")]
    ndt = new_ndt(pkg, refs("s-blobs"))
    n_two = run_sequence(pkg, O, refs, ndt, steps, HandleModel())
    assert n_two >= 5, n_two
    ndt.close()


@pytest.mark.gpu
def test_rebuilds_from_device_arrays(pkg, O, refs, hipmem):
    """setInputTargetDevice: the cloud already in HBM (structure of arrays)."""
    names = ["s-blobs", "s-blobs", "cells257", "s-neg", "crowded", "s-box-wide", "nan-exact-general", "s-blobs"]
    dev = {}
    for s in set(names):
        c = cloud(s)
        dev[s] = [hipmem.upload(np.ascontiguousarray(c[:, a])) for a in range(3)] + [len(c)]

    def load(s):
        return lambda _: ndt.setInputTargetDevice(*dev[s])
    ndt = new_ndt(pkg, refs("s-blobs"))
    steps = [(s, 1.0, 6, load(s)) for s in names]
    n_two = run_sequence(pkg, O, refs, ndt, steps, HandleModel())
    assert n_two >= 4, n_two
    ndt.close()


@pytest.mark.gpu
def test_rebuilds_through_the_asynchronous_hand_off(pkg, O, refs):
    """Host clouds in the 8-float point layout under the asynchronous hand-off, the two-launch build's partition
    launched chunk by chunk under the transfer."""
    names = ["s-blobs", "s-blobs", "n524289", "s-neg", "crowded", "s-lines", "n524289", "s-blobs"]

    def load(c):
        x = np.full((len(c), 8), 3.5, np.float32)
        x[:, :3] = c
        ndt.setInputTarget(x)
        x[:] = np.nan   # the hand-off has consumed the caller's array when setInputTarget returns
    with Tuned(pkg, handoff_chunk_pass=1):
        ndt = new_ndt(pkg, refs("s-blobs"))
        ndt.setHandoffMode(pkg.HANDOFF_ASYNC)
        steps = [(s, 1.0, 6, load) for s in names]
        n_two = run_sequence(pkg, O, refs, ndt, steps, HandleModel())
        assert n_two >= 4, n_two
        assert ndt.handoffCounters()[0] >= 1, ndt.handoffCounters()
        ndt.close()


@pytest.mark.gpu
def test_voxel_downsample_between_steady_state_builds(pkg, O, refs):
    """voxelDownsample runs the build's own kernels over the build's scratch buffers; the steady-state builds around
    it (and the dense index they reuse) are unaffected."""
    ndt = new_ndt(pkg, refs("s-blobs"))
    model = HandleModel()
    run_sequence(pkg, O, refs, ndt, [(s, 1.0, 6, "target") for s in ("s-lines", "s-blobs", "s-neg")], model)
    big = cloud("n1048577")
    assert len(ndt.voxelDownsample(big, 0.3)) > 100000
    n_two = run_sequence(pkg, O, refs, ndt, [(s, 1.0, 6, "target") for s in ("s-blobs", "s-lines", "s-blobs")], model)
    assert n_two == 3, n_two
    ndt.close()
