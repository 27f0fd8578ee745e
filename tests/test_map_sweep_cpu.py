"""The case generator of the voxel-map sweep (tests/test_gpu_map_sweep.py) and, without a GPU, the conditions that keep that
sweep from passing for the wrong reason.

Every kernel of the map family classifies a point by floorf(p * inv_leaf) in f32 with inv_leaf = 1.0f / leaf.  At a leaf
size with an exact inverse (1.0, 0.5, 0.25) dividing by the leaf, doing the product in f64 or taking a box edge with other
arithmetic than the add all give the same voxels; at the leaf sizes a map is run at they do not.  `cases()` therefore sweeps
leaf 0.1, 0.3, 0.7, 1.5 and 1.7 (0.5 as the one exact-inverse control) at four scene centres, five kinds of cloud scaled by
the leaf, five sizes, ragged pieces, non-finite rows, intensity, a grown table and moments on / off; every case with 700
points or more carries a FACE SET: points whose coordinates are f32(f32(k) * f32(leaf)) for voxel coordinates k within
+-30 of the centre's own voxel, the two f32 neighbours of each, and -0.0 at the origin.  The carve origin and the corners
of the crop / export boxes are points of that kind too.

Pinned here: the axes are covered; in every face set at least 100 points fall into another voxel under the f64 quotient
than under the f32 product (none at leaf 0.5); at least 20 box corners per inexact leaf do; the cases that build a target
yield at least 100 leaves and 500 pairs; `moments_numpy` + `leaves_from_moments` are the oracle's leaves bit for bit and
`voxelmap_numpy` is the dense index at the sweep's leaves (the bodies of the two tests that pin them at 1.0 / 0.5 and
0.5 / 0.3); every carve removes a voxel, keeps one and walks through a tie."""
import functools

import numpy as np
import pytest

from test_gpu_voxel_map import voxelmap_numpy
from test_map_carve_cpu import DEFAULTS, LIMIT, carve_numpy, to_grid, walk
from test_map_repose_cpu import rigid_pose
from test_map_state_cpu import mapstate_numpy
from test_map_target_cpu import cells_of, host_transform_f64, leaves_from_moments, moments_numpy, voxel_ijk
from test_voxel_map_cpu import voxelgrid_dense_numpy

LEAVES = (0.1, 0.3, 0.7, 1.5, 1.7, 0.5)                      # 0.5: inv_leaf = 2 exactly, the control
DYADIC = (0.5,)
CENTRES = ((0.0, 0.0, 0.0), (-37.5, 18.75, -3.75), (1500.0, -750.0, 150.0), (29000.0, 40.0, -5.0))
KINDS = ("blobs", "planes", "lines", "dupes", "box")
SIZES = (7, 60, 700, 5000, 20000)
CUTS = (257, 1, 0, 63, 64, 65, 4097)                         # piece sizes in add order (the first one carries the pose)
FACE_SPAN, FACE_POINTS, DUST_SPAN = 30, 600, 2
FACE_FACTOR = {1.5: 3}     # leaf 1.5 tells the two arithmetics apart least often (206 of 1 800 around the origin): a larger set
N_CASES = 36
SPECIAL_CARVE = dict(min_misses=1, keep_last=0, max_steps=7)


def cases():
    """36 seeded dicts.  Leaf, centre, kind and n are dealt so that every leaf meets every centre, every kind and every
    n; the two-valued axes are drawn from one seeded generator."""
    rng = np.random.default_rng(20250611)
    out = []
    for i in range(N_CASES):
        l, j = i % len(LEAVES), i // len(LEAVES)
        n = SIZES[(2 * j + l) % len(SIZES)]
        flags = rng.integers(0, 2, 8)
        out.append(dict(
            seed=7000 + i, leaf=LEAVES[l], centre=CENTRES[(j + l) % len(CENTRES)], kind=KINDS[(j + 2 * l) % len(KINDS)], n=n,
            bad=bool(flags[0]), intensity=bool(flags[1]), capacity=64 if flags[2] else 0,
            moments=bool(flags[3]) if n < 5000 else i % 7 != 3, pose=bool(flags[4]), remove_inside=int(flags[5]),
            carve_pose=bool(i % 2), carve_params=dict(SPECIAL_CARVE) if i in (8, 27) else {},
        ))
    return out


def case_id(c):
    return "%s-n%d-leaf%g-c%g%s%s%s%s" % (c["kind"], c["n"], c["leaf"], c["centre"][0], "-nan" if c["bad"] else "",
                                         "-int" if c["intensity"] else "", "-cap64" if c["capacity"] else "",
                                         "-mom" if c["moments"] else "")


def is_far(case):
    """beyond 1 km: translation-only poses (exact in f32), as test_gpu_build_paths.Ref does"""
    return float(np.abs(case["centre"]).max()) > 1000.0


def has_target(case):
    return case["moments"] and case["n"] >= 5000


# ---- face points ----------------------------------------------------------------------------------------------------------
def face_values(k, leaf):
    """f32(f32(k) * f32(leaf)) and its two f32 neighbours, for every k"""
    on = np.asarray(k).astype(np.float32) * np.float32(leaf)
    return np.concatenate([on, np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf))]).astype(np.float32)


def centre_voxel(case):
    return voxel_ijk(np.float32(case["centre"])[None], case["leaf"])[0]


def axis_faces(case, a, lo=-FACE_SPAN, hi=FACE_SPAN, base=None):
    base = centre_voxel(case) if base is None else base
    v = face_values(base[a] + np.arange(lo, hi + 1), case["leaf"])
    if case["centre"][a] == 0.0 and base[a] + lo <= 0 <= base[a] + hi:
        v = np.concatenate([v, np.float32([-0.0])])
    return v


def quotient_ijk(pts, leaf):
    """floor(f64(p) / f64(f32(leaf))): the voxel the exact quotient names"""
    return np.floor(np.asarray(pts, np.float32)[:, :3].astype(np.float64) / np.float64(np.float32(leaf))).astype(np.int64)


def mismatches(pts, leaf):
    """the points the f32 product puts into another voxel than the quotient"""
    return (quotient_ijk(pts, leaf) != voxel_ijk(pts, leaf)).any(axis=1)


def face_set(case, rng):
    m = FACE_POINTS * FACE_FACTOR.get(case["leaf"], 1)
    return np.stack([rng.choice(axis_faces(case, a), m) for a in range(3)], axis=1).astype(np.float32)


def face_corner(case, rng, base, lo, hi):
    """One face point with voxel offsets lo[a] .. hi[a] from the voxel `base`, on every axis a value that the product and
    the quotient floor differently; where the range holds none, it is widened away from `base` until it does (and where
    nothing within the face span does, any value of the range as given)."""
    out = np.zeros(3, np.float32)
    for a in range(3):
        for grow in range(FACE_SPAN):
            v = axis_faces(case, a, lo[a] - (grow if lo[a] < 0 else 0), hi[a] + (grow if lo[a] >= 0 else 0), base)
            p = np.zeros((len(v), 3), np.float32)
            p[:, 0] = v
            odd = v[mismatches(p, case["leaf"])]
            first = v if grow == 0 else first
            if len(odd) or case["leaf"] in DYADIC:
                break
        out[a] = rng.choice(odd if len(odd) else first)
    return out


def carve_origin(case, rng):
    """A face point within 2 voxels of the centre whose f32 product is a whole number on every axis: the ray starts on a
    voxel corner, so a ray that goes down on two axes meets two faces at t = 0 and the tie rule decides."""
    c = centre_voxel(case)
    out = np.zeros(3, np.float32)
    for a in range(3):
        v = face_values(c[a] + np.arange(-2, 3), case["leaf"])
        v = v[np.abs(v) > 0.5 * case["leaf"]]                 # (not the face at 0: no pose takes an f32 point back onto it)
        g = to_grid(v, case["leaf"])
        whole = v[g == np.floor(g)]
        out[a] = rng.choice(whole if len(whole) else v)
    return out


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def cloud_in_leaves(rng, kind, n):
    """The kinds of test_gpu_random.make_cloud in units of the leaf, [n, 3] f64: extents up to +-25 leaves in x, y and +-4 in
    z, thin structures with sigma 0.05 leaf, and as many voxels as give the well-filled ones six points and more."""
    big = n >= 20000
    if kind == "blobs":      # Gaussian clusters of about 100 points, sigma half a leaf
        c = rng.uniform(-1, 1, (max(1, n // 100), 3)) * [25.0, 25.0, 4.0]
        return c[rng.integers(0, len(c), n)] + rng.normal(0, 0.5, (n, 3))
    if kind == "planes":     # planes ON voxel faces (multiples of 3 leaves), straddled by their noise
        e = 6.0 if big else 4.0
        p = rng.uniform(-1, 1, (n, 3)) * [e, e, 4.0]
        k = rng.integers(0, 3, n)
        p[np.arange(n), k] = np.round(p[np.arange(n), k] / 3.0) * 3.0 + rng.normal(0, 0.05, n)
        return p
    if kind == "lines":      # three parallel lines: collinear voxels
        t = rng.uniform(-25, 25, n)
        d = rng.normal(size=3)
        d[2] *= 0.15
        d /= np.linalg.norm(d)
        return t[:, None] * d + rng.normal(0, 0.05, (n, 3)) + rng.integers(-1, 2, (n, 1)) * np.array([0.0, 1.7, 0.0])
    if kind == "dupes":      # every point eight times, every third row jittered
        e = np.array([6.0, 6.0, 4.0]) if big else np.array([3.0, 3.0, 3.0])
        q = rng.uniform(-1, 1, (max(1, n // 8), 3)) * e
        p = np.repeat(q, 8, axis=0)[:n]
        if len(p) < n:
            p = np.concatenate([p, q[:n - len(p)]])
        p[::3] += rng.normal(0, 0.05, p[::3].shape)
        return p
    e = 12.0 if big else 6.0 if n >= 5000 else 3.0           # uniform box, about nine points per voxel
    return rng.uniform(-1, 1, (n, 3)) * [e, e, 2.0]


def about_centre(case, T):
    """the pose T applied about the scene's centre"""
    c = np.asarray(case["centre"], np.float64)
    A, B = np.eye(4), np.eye(4)
    A[:3, 3], B[:3, 3] = c, -c
    return A @ T @ B


def small_pose(case, scale=1.0):
    """test_map_repose_cpu's general pose about the centre, its translation in leaves; beyond 1 km the translation alone"""
    t = np.array([10.3, -4.7, 0.21]) * case["leaf"] * scale
    if is_far(case):
        T = np.eye(4)
        T[:3, 3] = t
        return T
    return about_centre(case, rigid_pose(t=t))


def sensor_origin(pose, origin):
    """The f32 point of the sensor's frame that the pose takes back onto `origin` exactly, searched among the f32 neighbours
    of inv(pose) . origin; the nearest one if none does."""
    first = host_transform_f64(np.linalg.inv(pose), origin[None])[0]
    steps = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    cand = np.tile(first, (len(steps), 1))
    for _ in range(2):
        cand = np.where(steps > 0, np.nextafter(cand, np.float32(np.inf)), np.where(steps < 0, np.nextafter(cand, np.float32(-np.inf)), cand))
        steps = steps - np.sign(steps)
    back = host_transform_f64(pose, cand.astype(np.float32))
    miss = (back != origin).sum(axis=1) * 1e3 + np.abs(back.astype(np.float64) - origin).sum(axis=1)
    return cand[np.argmin(miss)].astype(np.float32)


@functools.lru_cache(maxsize=4)
def _make(index):
    case = cases()[index]
    leaf, centre = case["leaf"], np.asarray(case["centre"], np.float64)
    rng = np.random.default_rng(case["seed"])
    base = (cloud_in_leaves(rng, case["kind"], case["n"]) * leaf + centre).astype(np.float32)
    origin = carve_origin(case, rng)
    # dust: one point in each of the 4 x 4 x 4 voxels around the corner the carve origin stands on
    o = voxel_ijk(origin[None], leaf)[0]
    g = np.arange(-DUST_SPAN, DUST_SPAN)
    cell = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + o
    dust = ((cell + rng.uniform(0.3, 0.7, cell.shape)) * np.float64(np.float32(leaf))).astype(np.float32)
    parts, is_dust = [base, dust], [np.zeros(len(base), bool), np.ones(len(dust), bool)]
    faces = None
    if case["n"] >= 700:
        faces = face_set(case, rng)
        parts.append(faces)
        is_dust.append(np.zeros(len(faces), bool))
    xyz, is_dust = np.concatenate(parts), np.concatenate(is_dust)
    perm = rng.permutation(len(xyz))
    xyz, is_dust = np.ascontiguousarray(xyz[perm]), is_dust[perm]
    at = np.zeros(0, np.int64)
    if case["bad"]:
        at = rng.choice(np.nonzero(~is_dust)[0], min(5, case["n"] // 2), replace=False)
        rows = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [1, -np.inf, np.nan]])
        xyz[at] = xyz[at] + rows[:len(at)]                    # (a finite coordinate stays where it was)
    inten = rng.uniform(0, 255, len(xyz)).astype(np.float32) if case["intensity"] else None
    sizes = [s for s in CUTS if s <= case["n"] // 2]
    cuts = np.r_[0, np.cumsum(sizes), len(xyz)].astype(np.int64)
    pose = small_pose(case) if case["pose"] else None
    # what the map sees: every piece in order, then (with a pose) the first piece once more, moved
    seen, seen_i = xyz, inten
    if pose is not None:
        with np.errstate(invalid="ignore"):
            seen = np.concatenate([xyz, host_transform_f64(pose, xyz[:cuts[1]])])
        seen_i = None if inten is None else np.concatenate([inten, inten[:cuts[1]]])
    # boxes: corners are face points; the export box is the wider one
    # (placed around the carve origin's voxel, whose dust they split)
    box = (face_corner(case, rng, o, (-6, -6, -4), (-1, -1, -1)), face_corner(case, rng, o, (0, 0, 0), (5, 5, 3)))
    crop = (face_corner(case, rng, o, (-3, -3, -3), (-1, -1, -1)), face_corner(case, rng, o, (0, 0, 0), (2, 2, 2)))
    # rays: at most 3000 rows of the cloud -- rows that are not dust (the non-finite ones among them: skipped rays), and the
    # four dust points two voxels down from the origin's corner on x and on y: their rays leave the corner through two
    # faces at once
    cand = np.nonzero(~is_dust)[0]
    with np.errstate(invalid="ignore"):
        down = np.nonzero(is_dust & (voxel_ijk(xyz, leaf)[:, :2] == o[:2] - DUST_SPAN).all(axis=1))[0]
    cand = np.setdiff1d(cand, at)
    pick = np.sort(np.concatenate([rng.choice(cand, min(3000 - len(down) - len(at), len(cand)), replace=False), down, at]))
    rays, carve_pose, carve_org = xyz[pick].copy(), None, origin
    if case["carve_pose"]:                                    # the scan in the sensor's frame, the pose takes it to the map's
        carve_pose = small_pose(case, scale=-0.7)
        inv = np.linalg.inv(carve_pose)
        with np.errstate(invalid="ignore"):
            rays = host_transform_f64(inv, rays)
        carve_org = sensor_origin(carve_pose, origin)
    # a source for the target stage, as test_gpu_random builds it (translations in leaves)
    fin = seen[np.isfinite(seen).all(axis=1)]
    return dict(case=case, xyz=xyz, intensity=inten, cuts=cuts, pose=pose, seen=seen, seen_intensity=seen_i, faces=faces,
                box=box, crop=crop, origin=origin, rays=rays, carve_origin=carve_org, carve_pose=carve_pose,
                carve_params=dict(DEFAULTS, **case["carve_params"]), finite=fin)


def make_case(case):
    """The clouds of one case: dict(xyz [m, 3] f32 in add order, intensity [m] or None, cuts (piece k is rows cuts[k] ..
    cuts[k + 1]), pose (4 x 4, or None: the first piece is added once more under it), seen / seen_intensity (everything the
    map was given, in order), faces (the face set, or None), box / crop (two face-point corners each), origin (the carve
    origin in the map's frame, a face point), rays, carve_origin, carve_pose (what mapCarve is given), carve_params)."""
    return _make(cases().index(case))


def pieces_of(d):
    cloud = d["xyz"] if d["intensity"] is None else np.concatenate([d["xyz"], d["intensity"][:, None]], axis=1)
    return [np.ascontiguousarray(cloud[a:b]) for a, b in zip(d["cuts"][:-1], d["cuts"][1:])]


def source_of(d, S, O):
    """(source cloud, poses [2, 6]: the near pose and the identity) as test_gpu_random builds them, translations in leaves"""
    case = d["case"]
    rng = np.random.default_rng(case["seed"] + 500)
    leaf, tgt = case["leaf"], d["finite"]
    rot = np.zeros(3) if is_far(case) else rng.normal(0, 0.01, 3)
    dT = S.pose_matrix(*(rng.normal(0, 0.05 * leaf, 3)), *rot)
    if not is_far(case):
        dT = about_centre(case, dT)
    src = S.transform(np.linalg.inv(dT), tgt[rng.random(len(tgt)) < 0.7].astype(np.float64)).astype(np.float32)
    src = np.concatenate([src, (rng.uniform(-60, 60, (5, 3)) * leaf + case["centre"]).astype(np.float32)])
    return src, np.stack([O.matrix_to_pose(dT), np.zeros(6)])


def target_kw(case):
    return dict(resolution=case["leaf"], step_size=0.1, trans_epsilon=1e-4, max_iterations=20)


def ties_on_walk(gs, ge):
    """The steps of test_map_carve_cpu.walk at which the smallest tMax is shared by two axes or more (the tie rule
    decides); the path is walk()'s own."""
    gs, ge = [float(v) for v in gs], [float(v) for v in ge]
    v, ve = [int(np.floor(g)) for g in gs], [int(np.floor(g)) for g in ge]
    inf = float("inf")
    step, tdelta, tmax = [0] * 3, [0.0] * 3, [inf] * 3
    for a in range(3):
        if ve[a] != v[a]:
            d = ge[a] - gs[a]
            step[a] = 1 if ve[a] > v[a] else -1
            tdelta[a] = 1.0 / abs(d)
            tmax[a] = (float(v[a] + (1 if step[a] > 0 else 0)) - gs[a]) / d
    path, ties = [tuple(v)], 0
    for _ in range(sum(abs(ve[a] - v[a]) for a in range(3))):
        a = 0 if tmax[0] <= tmax[1] and tmax[0] <= tmax[2] else 1 if tmax[1] <= tmax[2] else 2
        ties += sum(1 for b in range(3) if tmax[b] == tmax[a]) > 1
        v[a] += step[a]
        tmax[a] = inf if v[a] == ve[a] else tmax[a] + tdelta[a]
        path.append(tuple(v))
    assert path == walk(gs, ge)
    return ties


# ---- the conditions ---------------------------------------------------------------------------------------------------------
def test_cases_are_deterministic_and_cover_the_axes():
    cs = cases()
    assert repr(cs) == repr(cases()) and len(cs) == N_CASES and len({case_id(c) + str(c["seed"]) for c in cs}) == N_CASES
    assert {c["leaf"] for c in cs} == set(LEAVES) and {c["centre"] for c in cs} == set(CENTRES)
    for leaf in LEAVES:
        mine = [c for c in cs if c["leaf"] == leaf]
        assert {c["centre"] for c in mine} == set(CENTRES), leaf
        assert {c["kind"] for c in mine} == set(KINDS), leaf
        assert {c["n"] for c in mine} == set(SIZES), leaf
        assert any(has_target(c) for c in mine), leaf
    for centre in CENTRES:
        assert any(has_target(c) for c in cs if c["centre"] == centre), centre
    for key in ("bad", "intensity", "capacity", "moments", "pose", "remove_inside", "carve_pose"):
        on = sum(bool(c[key]) for c in cs)
        assert 8 <= on <= N_CASES - 8, (key, on)
    assert sum(bool(c["carve_params"]) for c in cs) == 2
    # the pieces: 1, 63, 64, 65, 257 and 4097 where n allows, and an empty one
    for c in cs:
        d = make_case(c)
        sizes = np.diff(d["cuts"]).tolist()
        assert sum(sizes) == len(d["xyz"]) and 0 in sizes and 1 in sizes
        for s in (63, 64, 65, 257, 4097):
            assert (s in sizes) == (s <= c["n"] // 2), (case_id(c), s)
        assert (d["faces"] is not None) == (c["n"] >= 700)
        assert np.isfinite(d["xyz"]).all() != c["bad"]
        again = _make.__wrapped__(cs.index(c))
        assert np.array_equal(again["xyz"].view(np.uint32), d["xyz"].view(np.uint32)) and np.array_equal(again["rays"].view(np.uint32), d["rays"].view(np.uint32))
    assert any(4097 in np.diff(make_case(c)["cuts"]) for c in cs)


def test_face_sets_tell_the_product_from_the_quotient():
    """In every face set at least 100 of the 600 points are in another voxel under the quotient; at leaf 0.5 none is."""
    worst = {}
    for c in cases():
        d = make_case(c)
        if d["faces"] is None:
            continue
        odd = int(mismatches(d["faces"], c["leaf"]).sum())
        in_cloud = int(mismatches(d["finite"], c["leaf"]).sum())
        print("face set %-44s %4d of %d face points (%d of the %d finite points the map sees)"
              % (case_id(c), odd, len(d["faces"]), in_cloud, len(d["finite"])))
        if c["leaf"] in DYADIC:
            assert odd == 0 and in_cloud == 0, case_id(c)
        else:
            assert odd >= 100, (case_id(c), odd)
            worst[c["leaf"]] = min(worst.get(c["leaf"], odd), odd)
        # the face points are what they claim: on a face or one f32 step beside it, within +-30 voxels of the centre
        k = np.round(d["faces"].astype(np.float64) / np.float64(np.float32(c["leaf"])))
        on = (k.astype(np.float32) * np.float32(c["leaf"])).astype(np.float32)
        near = (d["faces"] == on) | (d["faces"] == np.nextafter(on, np.float32(-np.inf))) | (d["faces"] == np.nextafter(on, np.float32(np.inf)))
        assert near.all() and (np.abs(k - centre_voxel(c)) <= FACE_SPAN).all()
    for leaf in sorted(worst):
        print("leaf %g: the smallest face-mismatch count of a case is %d" % (leaf, worst[leaf]))
    print("the smallest over the sweep: %d of %d" % (min(worst.values()), FACE_POINTS))
    assert set(worst) == set(LEAVES) - set(DYADIC)


def test_box_corners_tell_the_product_from_the_quotient():
    count = {leaf: [0, 0] for leaf in LEAVES}
    for c in cases():
        d = make_case(c)
        corners = np.stack([*d["box"], *d["crop"]])
        assert (corners[0] < corners[1]).all() and (corners[2] < corners[3]).all()
        odd = mismatches(corners, c["leaf"])
        count[c["leaf"]][0] += int(odd.sum())
        count[c["leaf"]][1] += len(corners)
        # each box splits the map: voxels inside and outside
        st_ijk = np.unique(voxel_ijk(d["finite"], c["leaf"]), axis=0)
        for lo, hi in (d["box"], d["crop"]):
            inside = ((st_ijk >= voxel_ijk(lo[None], c["leaf"])[0]) & (st_ijk <= voxel_ijk(hi[None], c["leaf"])[0])).all(axis=1)
            assert 0 < inside.sum() < len(inside), case_id(c)
    for leaf, (odd, n) in count.items():
        print("leaf %g: %d of %d box corners floor differently under the f32 product and the f64 quotient" % (leaf, odd, n))
        assert (odd == 0) if leaf in DYADIC else (odd >= 20), (leaf, odd)


def test_the_sparse_yardstick_agrees_with_the_dense_index_on_every_case():
    """The body of test_voxel_map_cpu.test_the_sparse_yardstick_agrees_with_the_dense_index on the sweep's clouds."""
    ran = 0
    for c in cases():
        d = make_case(c)
        leaf = c["leaf"]
        ijk = voxel_ijk(d["finite"], leaf)
        if np.prod((ijk.max(0) - ijk.min(0) + 1).astype(np.float64)) >= 2**31 - 1:
            continue
        xyz, _, counts, ijk = voxelmap_numpy(d["seen"], leaf)
        dense, dcounts = voxelgrid_dense_numpy(d["seen"], leaf)
        assert np.array_equal(xyz.view(np.uint32), dense.view(np.uint32)) and np.array_equal(counts, dcounts), case_id(c)
        assert np.array_equal(ijk, ijk[np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))]) and len(np.unique(ijk, axis=0)) == len(ijk)
        ran += 1
    assert ran == N_CASES                                     # every dense index fits


TARGET_CASES = [c for c in cases() if has_target(c)]


@pytest.mark.parametrize("case", TARGET_CASES, ids=case_id)
def test_sequential_f64_sums_are_the_oracles_leaves_bit_for_bit(O, S, case):
    """The body of test_map_target_cpu's test of the same name at the sweep's leaves and centres, face points in the cloud;
    plus what the target stage of the GPU sweep needs: 100 leaves, and 500 pairs at the near pose."""
    d = make_case(case)
    leaf, cloud = case["leaf"], d["seen"]
    prm = O.default_params(num_threads=4, **target_kw(case))
    grid = O.Grid(cloud, prm)
    OL = grid.export()
    ijk, count, sums = moments_numpy(cloud, leaf)
    assert np.array_equal(ijk.min(0), grid.min_b) and np.array_equal(ijk.max(0), grid.max_b)
    min_pts = max(3, prm.min_points_per_voxel)
    keep, mean, cov = leaves_from_moments(ijk, count, sums, min_pts)
    cell = cells_of(ijk[keep], grid.min_b, grid.div_b)
    # the oracle exports the leaves that passed its validity checks: every one of them is a candidate, in cell order
    at = np.searchsorted(cell, OL["cell"])
    assert np.array_equal(cell[at], OL["cell"])
    assert np.array_equal(count[keep][at], OL["count"])
    assert np.array_equal(mean[at], OL["mean"])                                   # bit for bit
    # a leaf whose two small eigenvalues stand above the inflation floor keeps its covariance as computed
    plain = OL["evals"][:, 0] > prm.eig_inflation_ratio * OL["evals"][:, 2] * (1 + 1e-9)
    assert plain.sum() > 20
    assert np.array_equal(cov[at][plain], OL["cov"][plain])                       # bit for bit
    src, poses = source_of(d, S, O)
    e = grid.derivatives(src, poses[0], params=O.default_params(num_threads=4, search_method=O.DIRECT7, **target_kw(case)))
    print("target %-44s %5d leaves (%d un-inflated), %6d pairs under DIRECT7 at the near pose"
          % (case_id(case), grid.n_leaves, plain.sum(), e["n_pairs"]))
    assert grid.n_leaves >= 100 and e["n_pairs"] >= 500


def test_every_carve_removes_keeps_and_walks_through_a_tie():
    for c in cases():
        d = make_case(c)
        leaf = c["leaf"]
        st = mapstate_numpy(d["seen"], leaf)
        want = carve_numpy(st["ijk"], st["count"], d["rays"], d["carve_origin"], leaf, d["carve_pose"], **d["carve_params"])
        assert want["n_removed"] >= 1 and want["keep"].sum() >= 1, (case_id(c), want["n_removed"])
        assert want["n_rays"] == len(d["rays"]) <= 3000 and want["n_rays_skipped"] < want["n_rays"]
        if c["bad"]:
            assert want["n_rays_skipped"] >= 1
        # the origin the map sees is a face point, or (under the pose) within a few f32 steps of one
        o, pts = d["carve_origin"][None], d["rays"]
        if d["carve_pose"] is not None:
            with np.errstate(invalid="ignore"):
                o, pts = host_transform_f64(d["carve_pose"], o), host_transform_f64(d["carve_pose"], pts)
            assert (np.abs(o[0] - d["origin"]) <= 4 * np.spacing(np.abs(d["origin"]).max().astype(np.float32))).all()
        gs, ge = to_grid(o, leaf)[0], to_grid(pts, leaf)
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(d["rays"]).all(axis=1) & np.isfinite(ge).all(axis=1) & (np.abs(np.floor(ge)) < LIMIT).all(axis=1)
        first = next((r for r, g in enumerate(ge[ok]) if ties_on_walk(gs, g) > 0), None)
        print("carve %-44s %4d rays, %3d removed of %5d voxels, the first ray that walks through a tie is ray %s"
              % (case_id(c), want["n_rays"], want["n_removed"], len(st["count"]), first))
        assert first is not None, case_id(c)
