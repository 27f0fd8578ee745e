"""getFitnessScore on the GPU (ndt_fitness_score / ndt_fitness_scores) against an exact CPU nearest-neighbour search:
scipy's cKDTree in f64 over the finite target points, queried with the points ndt_transform_source returns for the
same transform -- so only the search and the sums are under test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = np.finfo(np.float64).max
RANGES = (DBL_MAX, 0.01, 0.25, 1.0, 4.0)

pytestmark = pytest.mark.gpu


def ref_sq_dists(target, q):
    """f64 d^2 from every finite query point to the nearest finite target point (NaN for a non-finite query)."""
    from scipy.spatial import cKDTree
    t = np.asarray(target, np.float64)[:, :3]
    t = t[np.isfinite(t).all(1)]
    out = np.full(len(q), np.nan)
    fin = np.isfinite(q).all(1)
    d, _ = cKDTree(t).query(np.asarray(q, np.float64)[fin], workers=16)
    out[fin] = d * d
    return out


def check_against(ref, got, sq=None, max_range=DBL_MAX):
    """got: fitness dict; ref: f64 d^2 per source point; sq: the per-point output (max_range = DBL_MAX) or None."""
    fin = np.isfinite(ref)
    assert got["n_points"] == int(fin.sum())
    d = ref[fin]
    if sq is not None:
        assert np.array_equal(np.isnan(sq), ~fin)
        s = sq[fin].astype(np.float64)
        if max_range == DBL_MAX:
            assert np.all(np.abs(s - d) <= 1e-5 * d + 1e-9), np.max(np.abs(s - d) / np.maximum(d, 1e-12))
    inl = d <= max_range
    near = np.abs(d - max_range) <= 1e-5 * max_range
    assert abs(got["n_inliers"] - int(inl.sum())) <= int(near.sum())
    if int(inl.sum()) == 0 and not near.any():
        assert got["n_inliers"] == 0 and got["fitness_score"] == DBL_MAX and got["sum_sq_dist"] == 0.0
        return
    ref_sum = float(d[inl].sum())
    slack = float(d[near].sum())
    assert abs(got["sum_sq_dist"] - ref_sum) <= 1e-6 * ref_sum + slack + 1e-12
    if not near.any():
        assert got["n_inliers"] == int(inl.sum())
        assert abs(got["fitness_score"] - ref_sum / inl.sum()) <= 1e-6 * (ref_sum / inl.sum()) + 1e-15


def engine(pkg, res, **kw):
    return pkg.NormalDistributionsTransform(device_id=0, resolution=res, step_size=0.1, trans_epsilon=1e-4,
                                            max_iterations=50, **kw)


def check_pose(ndt, target, T, ranges=RANGES):
    q = ndt.transformSource(T)
    ref = ref_sq_dists(target, q)
    got = ndt.fitness(T, per_point=True)
    check_against(ref, got, got["sq_dists"])
    for r in ranges:
        if r != DBL_MAX:
            g = ndt.fitness(T, max_range=r, per_point=True)
            check_against(ref, g, None, r)
            sq = g["sq_dists"]
            fin = np.isfinite(ref)
            # +INF exactly where d^2 > max_range (boundary points either way)
            far = ref[fin] > r * (1 + 1e-5)
            close = ref[fin] < r * (1 - 1e-5)
            assert np.all(np.isinf(sq[fin][far])) and np.all(np.isfinite(sq[fin][close]))
    return ref, got


@pytest.mark.parametrize("name", ["c1", "c2", "c3"])
def test_configs_at_guess_and_aligned_pose(pkg, S, name):
    cfg = {"c1": S.config_c1, "c2": S.config_c2, "c3": S.config_c3}[name]()
    ndt = engine(pkg, cfg["resolution"])
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    check_pose(ndt, cfg["target"], cfg["guess"])
    T = ndt.align(cfg["guess"])
    ref, got = check_pose(ndt, cfg["target"], T)
    assert ndt.getFitnessScore() == got["fitness_score"]          # the last align's final transformation
    assert ndt.getFitnessScore(1.0) == ndt.fitness(T, max_range=1.0)["fitness_score"]
    # a range that admits no point
    g = ndt.fitness(T, max_range=0.0)
    if np.nanmin(ref) > 0:
        assert g["n_inliers"] == 0 and g["fitness_score"] == DBL_MAX
    ndt.close()


def test_identity_before_any_align(pkg, S):
    cfg = S.config_c1()
    ndt = engine(pkg, 1.0)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    assert ndt.getFitnessScore() == ndt.fitness(np.eye(4))["fitness_score"]
    ndt.close()


@pytest.mark.parametrize("shift", [50.0, 500.0])
def test_source_far_off_the_map(pkg, S, shift):
    cfg = S.config_c1()
    ndt = engine(pkg, 1.0)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    T = np.array(cfg["guess"], np.float64)
    T[:3, 3] += np.array([shift, 0.3 * shift, -0.2 * shift])
    check_pose(ndt, cfg["target"], T, ranges=(DBL_MAX, 1.0, shift * shift))
    ndt.close()
    # a scan-sized map, a subsample of the scan 50 m off to the side
    cfg = S.config_c2()
    ndt = engine(pkg, 1.0)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"][::64])
    T = np.eye(4)
    T[:3, 3] = [0.0, 50.0 if shift == 50.0 else 0.0, 0.0 if shift == 50.0 else 30.0]
    check_pose(ndt, cfg["target"], T, ranges=(DBL_MAX, 4.0))
    ndt.close()


def test_km_scale_coordinates(pkg, S):
    cfg = S.config_c1()
    off = np.array([3000.0, 3000.0, 0.0], np.float32)
    tgt = (cfg["target"] + off).astype(np.float32)
    src = (cfg["source"] + off).astype(np.float32)
    ndt = engine(pkg, 1.0)
    ndt.setInputTarget(tgt)
    ndt.setInputSource(src)
    check_pose(ndt, tgt, np.eye(4))
    T = np.eye(4)
    T[:3, 3] = [0.37, -0.21, 0.11]
    check_pose(ndt, tgt, T)
    ndt.close()


def test_c3_wide(pkg, S):
    cfg = S.config_c3_wide()
    ndt = engine(pkg, cfg["resolution"])
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    check_pose(ndt, cfg["target"], cfg["guess"], ranges=(DBL_MAX, 0.25))
    ndt.close()


def test_sparse_duplicate_and_nonfinite_points(pkg, S):
    rng = np.random.default_rng(5)
    cfg = S.config_c1()
    tgt = cfg["target"].astype(np.float32).copy()
    # isolated points: voxels below min_points_per_voxel (no leaf), still candidates
    iso = rng.uniform(-30, 30, (40, 3)).astype(np.float32)
    dup = np.repeat(tgt[:50], 4, axis=0)
    bad = np.array([[np.nan, 0, 0], [np.inf, 1, 1], [0, -np.inf, 2], [1e3, np.nan, np.nan]], np.float32)
    tgt = np.concatenate([tgt[:3000], bad, iso, dup, tgt[3000:], bad])
    src = cfg["source"].astype(np.float32).copy()
    src[::97] = np.nan
    src[5] = [np.inf, 0, 0]
    src = np.concatenate([src, iso + 0.01, iso[:5]])          # points right at (and on) the isolated ones
    ndt = engine(pkg, 1.0)
    ndt.setInputTarget(tgt)
    ndt.setInputSource(src)
    ref, got = check_pose(ndt, tgt, cfg["guess"])
    assert got["n_points"] == int(np.isfinite(ref).sum()) < len(src)
    ref, got = check_pose(ndt, tgt, np.eye(4))
    assert np.all(got["sq_dists"][-5:] == 0.0)                 # exact duplicates of target points
    ndt.close()


def test_target_inputs(pkg, S, hipmem):
    cfg = S.config_c1()
    tgt = cfg["target"].astype(np.float32)
    L = pkg.lib()
    ndt = engine(pkg, 1.0)
    ndt.setInputSource(cfg["source"])
    # AoS, 32-byte stride (pcl::PointXYZI)
    aos = np.zeros((len(tgt), 8), np.float32)
    aos[:, :3] = tgt
    assert L.ndt_set_target(ndt._h, aos.ctypes.data, len(aos), 32) == 0
    a = ndt.fitness(cfg["guess"])
    check_against(ref_sq_dists(tgt, ndt.transformSource(cfg["guess"])), a)
    # SoA
    ndt.setInputTargetSoA(tgt[:, 0], tgt[:, 1], tgt[:, 2])
    assert ndt.fitness(cfg["guess"]) == a
    # keyframe-assembled: two halves, one moved by a pose that the other half's points undo
    P = np.eye(4)
    P[:3, 3] = [1.0, -2.0, 0.5]
    h = len(tgt) // 2
    ndt.putKeyframe(1, tgt[:h])
    ndt.putKeyframe(2, (tgt[h:] - P[:3, 3]).astype(np.float32))
    ndt.setInputTargetFromKeyframes([1, 2], [np.eye(4), P])
    kf_tgt = np.concatenate([tgt[:h], ((tgt[h:] - P[:3, 3]).astype(np.float32) + P[:3, 3]).astype(np.float32)])
    check_against(ref_sq_dists(kf_tgt, ndt.transformSource(cfg["guess"])), ndt.fitness(cfg["guess"]))
    # device-consumed target: nothing retained
    d = [hipmem.upload(np.ascontiguousarray(tgt[:, i])) for i in range(3)]
    ndt.setInputTargetDevice(d[0], d[1], d[2], len(tgt))
    with pytest.raises(pkg.NdtError) as ei:
        ndt.fitness(cfg["guess"])
    assert ei.value.code == -9
    ndt.close()
    # multi-grid target
    ndt = engine(pkg, 1.0)
    ndt.setInputSource(cfg["source"])
    ndt.addTarget(tgt[:h], 1)
    ndt.addTarget(tgt[h:], 2)
    ndt.createVoxelKdtree()
    with pytest.raises(pkg.NdtError) as ei:
        ndt.fitness(cfg["guess"])
    assert ei.value.code == -9
    ndt.close()


def test_errors(pkg, S):
    cfg = S.config_c1()
    ndt = engine(pkg, 1.0)
    with pytest.raises(pkg.NdtError) as ei:
        ndt.fitness(np.eye(4))
    assert ei.value.code == -4
    ndt.setInputTarget(cfg["target"])
    with pytest.raises(pkg.NdtError) as ei:
        ndt.fitness(np.eye(4))
    assert ei.value.code == -5
    ndt.setInputSource(cfg["source"])
    for bad in (-1.0, float("nan")):
        with pytest.raises(pkg.NdtError) as ei:
            ndt.fitness(np.eye(4), max_range=bad)
        assert ei.value.code == -1
    L = pkg.lib()
    f = pkg.Fitness()
    T = np.eye(4, dtype=np.float32)
    sq = np.zeros(10, np.float32)
    assert L.ndt_fitness_score(ndt._h, T.ctypes.data_as(C.POINTER(C.c_float)), DBL_MAX, C.byref(f),
                               sq.ctypes.data_as(C.POINTER(C.c_float)), 10) == -1
    assert L.ndt_fitness_scores(ndt._h, T.ctypes.data_as(C.POINTER(C.c_float)), 0, DBL_MAX, C.byref(f)) == -1
    assert pkg.lib().ndt_last_error(ndt._h)
    ndt.close()


def test_cache_follows_the_target(pkg, S):
    cfg = S.config_c1()
    tgt = cfg["target"].astype(np.float32)
    ndt = engine(pkg, 1.0)
    ndt.setInputTarget(tgt)
    ndt.setInputSource(cfg["source"])
    a = ndt.fitness(cfg["guess"])
    tgt2 = (tgt[::3] + np.float32(0.05)).astype(np.float32)
    ndt.setInputTarget(tgt2)
    b = ndt.fitness(cfg["guess"])
    check_against(ref_sq_dists(tgt2, ndt.transformSource(cfg["guess"])), b)
    assert b != a
    # a resolution change re-voxelises the same points: the index is rebuilt at another cell edge, same answer
    ndt.setResolution(0.37)
    c = ndt.fitness(cfg["guess"])
    check_against(ref_sq_dists(tgt2, ndt.transformSource(cfg["guess"])), c)
    ndt.setResolution(3.0)
    assert ndt.fitness(cfg["guess"]) == c
    ndt.close()


def test_async_handoff_orders_fitness_behind_the_upload(pkg, S):
    cfg = S.config_c3()
    ndt = engine(pkg, cfg["resolution"])
    ndt.setHandoffMode(pkg.HANDOFF_ASYNC)
    ndt.setInputSource(cfg["source"])
    ndt.setInputTarget(cfg["target"][::2])
    ndt.fitness(cfg["guess"])
    ndt.setInputTarget(cfg["target"])
    got = ndt.fitness(cfg["guess"], per_point=True)         # right behind the upload and the pending build
    check_against(ref_sq_dists(cfg["target"], ndt.transformSource(cfg["guess"])), got, got["sq_dists"])
    ndt.close()


def test_bit_reproducible(pkg, S, hipmem):
    cfg = S.config_c3()
    src = cfg["source"].astype(np.float32)
    ndt = engine(pkg, cfg["resolution"])
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(src)
    T = cfg["guess"]
    runs = [ndt.fitness(T, max_range=1.0, per_point=True) for _ in range(3)]
    for r in runs[1:]:
        assert r["sq_dists"].tobytes() == runs[0]["sq_dists"].tobytes()
        assert {k: v for k, v in r.items() if k != "sq_dists"} == {k: v for k, v in runs[0].items() if k != "sq_dists"}
    base = {k: v for k, v in runs[0].items() if k != "sq_dists"}
    for order in (pkg.SOURCE_ORDER_AUTO, pkg.SOURCE_ORDER_KEEP, pkg.SOURCE_ORDER_SORT):
        ndt.setParams(source_order=order)
        ndt.align(T)
        assert ndt.fitness(T, max_range=1.0) == base
    # a fresh index over the same target (new handle) and a viewed source
    ndt2 = engine(pkg, cfg["resolution"])
    ndt2.setInputTarget(cfg["target"])
    d = [hipmem.upload(np.ascontiguousarray(src[:, i])) for i in range(3)]
    ndt2.setInputSourceDeviceView(d[0], d[1], d[2], len(src))
    assert ndt2.fitness(T, max_range=1.0) == base
    ndt2.close()
    # K = 8 poses in one launch == 8 single calls
    rng = np.random.default_rng(3)
    Ts = []
    for k in range(8):
        P = np.array(T, np.float64)
        P[:3, 3] += rng.normal(0, 0.3, 3)
        Ts.append(P)
    many = ndt.fitnessMany(Ts, max_range=1.0)
    assert many == [ndt.fitness(P, max_range=1.0) for P in Ts]
    many = ndt.fitnessMany(Ts)
    assert many == [ndt.fitness(P) for P in Ts]
    ndt.close()


CPP = r"""
#include <cstdio>
#include <vector>
#if FACE_COMPAT
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <pcl/registration/registration.h>
#include <pclomp/ndt_omp.h>
#include <pclomp/ndt_omp_impl.hpp>
using PointT = pcl::PointXYZI;
using Cloud = pcl::PointCloud<PointT>;
using Ndt = pclomp::NormalDistributionsTransform<PointT, PointT>;
#else
#include "ndt_hip/ndt_hip.hpp"
using PointT = ndt_hip::PointXYZ;
using Cloud = ndt_hip::PointCloud<PointT>;
using Ndt = ndt_hip::NormalDistributionsTransform<PointT, PointT>;
#endif

static bool load(const char* path, Cloud& c) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  long long n = 0;
  if (std::fread(&n, 8, 1, f) != 1) return false;
  std::vector<float> xyz(3 * n);
  if (std::fread(xyz.data(), 4, xyz.size(), f) != xyz.size()) return false;
  std::fclose(f);
  c.points.resize(n);
  for (long long i = 0; i < n; ++i) {
    c.points[i].x = xyz[3 * i]; c.points[i].y = xyz[3 * i + 1]; c.points[i].z = xyz[3 * i + 2];
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  typename Cloud::Ptr tgt(new Cloud()), src(new Cloud());
  if (!load(argv[1], *tgt) || !load(argv[2], *src)) return 3;
  Ndt ndt;
  if (ndt.lastStatus() != 0) return 4;
  ndt.setResolution(1.0f);
  ndt.setMaximumIterations(50);
  ndt.setTransformationEpsilon(1e-4);
  ndt.setStepSize(0.1);
  std::printf("before %.17g\n", ndt.getFitnessScore());
  ndt.setInputTarget(tgt);
  ndt.setInputSource(src);
  std::printf("identity %.17g\n", ndt.getFitnessScore());
  float g[16];
  FILE* f = std::fopen(argv[3], "rb");
  if (!f || std::fread(g, 4, 16, f) != 16) return 5;
  std::fclose(f);
  ndt_hip::Matrix4f guess;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) guess(r, c) = g[4 * c + r];
  Cloud out;
  ndt.align(out, guess);
  const ndt_hip::Matrix4f T = ndt.getFinalTransformation();
  std::printf("T");
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) std::printf(" %.9g", (double)T(r, c));
  std::printf("\nfitness %.17g\nranged %.17g\nstatus %d\n", ndt.getFitnessScore(), ndt.getFitnessScore(0.25),
              ndt.lastStatus());
  return 0;
}
"""


@pytest.mark.parametrize("face", ["plain", "compat"])
def test_cpp_adapter_get_fitness_score(pkg, S, tmp_path, face):
    cfg = S.config_c1()
    for name, a in (("tgt.bin", cfg["target"]), ("src.bin", cfg["source"])):
        a = np.ascontiguousarray(a, np.float32)
        with open(tmp_path / name, "wb") as f:
            f.write(np.int64(len(a)).tobytes() + a.tobytes())
    (tmp_path / "guess.bin").write_bytes(np.ascontiguousarray(np.asarray(cfg["guess"], np.float32).T).tobytes())
    (tmp_path / "fit.cpp").write_text(CPP)
    inc = ["-I" + os.path.join(ROOT, "tests", "cpp", "mock"), "-I" + os.path.join(ROOT, "include", "compat"),
           "-I" + os.path.join(ROOT, "include")]
    if face == "plain":
        inc = ["-DNDT_HIP_WITH_EIGEN=0", "-DNDT_HIP_WITH_PCL=0", "-DNDT_HIP_WITH_GTSAM=0", "-DFACE_COMPAT=0"] + inc[2:]
    else:
        inc = ["-DFACE_COMPAT=1"] + inc
    lib = os.path.join(ROOT, "slam-sam_amd", "libndt_hip.so")
    exe = str(tmp_path / "fit")
    subprocess.run(["g++", "-O2", "-std=c++20", "-Wall"] + inc + ["-o", exe, str(tmp_path / "fit.cpp"), lib,
                    "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=300)
    p = subprocess.run([exe, str(tmp_path / "tgt.bin"), str(tmp_path / "src.bin"), str(tmp_path / "guess.bin")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    vals = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines()}
    assert float(vals["before"][0]) == DBL_MAX                    # no target yet: DBL_MAX, lastStatus set
    T = np.array([float(v) for v in vals["T"]], np.float32).reshape(4, 4).T
    ndt = engine(pkg, 1.0)
    ndt.setInputTarget(cfg["target"])
    ndt.setInputSource(cfg["source"])
    assert float(vals["identity"][0]) == ndt.fitness(np.eye(4))["fitness_score"]
    assert float(vals["fitness"][0]) == ndt.fitness(T)["fitness_score"]
    assert float(vals["ranged"][0]) == ndt.fitness(T, max_range=0.25)["fitness_score"]
    assert int(vals["status"][0]) == 0
    ndt.close()
