// The C++ adapter's re-pose surface (mapTransform / mapImportStatePosed) with PCL-typed clouds and the pose types a
// driver holds (Eigen::Matrix4d, gtsam::Pose3; API mocks, tests/cpp/mock): after a loop closure the map, or a submap's
// saved state, is moved by the corrected pose.  The scene is a lattice one -- leaf 0.5, points on multiples of 1/64
// strictly inside their voxels, a few dozen per voxel -- and the poses are symmetries of the lattice, so every sum is exact
// and the moved map must equal, bit for bit, a map that was fed the moved points.
// Needs a GPU.  Prints "map repose: PASS" and returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/ndt_omp.h>

#include <gtsam/geometry/Pose3.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static bool same_state(const ndt_hip::MapState& a, const ndt_hip::MapState& b) {
  return a.leaf == b.leaf && a.ijk == b.ijk && a.counts == b.counts && a.sums.size() == b.sums.size() &&
         a.moments.size() == b.moments.size() &&
         (a.sums.empty() || std::memcmp(a.sums.data(), b.sums.data(), a.sums.size() * sizeof(float)) == 0) &&
         (a.moments.empty() || std::memcmp(a.moments.data(), b.moments.data(), a.moments.size() * sizeof(double)) == 0);
}

using Point = pcl::PointXYZ;
using Cloud = pcl::PointCloud<Point>;
using Ndt = pclomp::NormalDistributionsTransform<Point, Point>;

static Cloud moved(const Cloud& in, const Eigen::Matrix4d& T) {
  Cloud out;
  for (const auto& p : in.points) {
    Point q{};
    const double v[3] = {p.x, p.y, p.z};
    double w[3];
    for (int a = 0; a < 3; ++a) w[a] = ((T(a, 0) * v[0] + T(a, 1) * v[1]) + T(a, 2) * v[2]) + T(a, 3);   // exact on the lattice
    q.x = (float)w[0]; q.y = (float)w[1]; q.z = (float)w[2];
    out.points.push_back(q);
  }
  return out;
}

static void fresh_map(Ndt& n, float leaf) {
  n.setResolution(leaf);
  n.mapReset(leaf, false, 64);
  n.mapEnableMoments();
}

int main() {
  const float leaf = 0.5f;
  // 300 voxels inside |x| < 20, 1 .. 40 points each
  std::mt19937 rng(21);
  std::uniform_int_distribution<int> uv(-40, 39), un(1, 40), uin(1, 31);
  std::set<std::array<int, 3>> voxels;
  while (voxels.size() < 300) voxels.insert({uv(rng), uv(rng), uv(rng)});
  Cloud scene;
  for (const auto& v : voxels)
    for (int k = un(rng); k > 0; --k) {
      Point p{};
      p.x = (float)(v[0] * 0.5 + uin(rng) / 64.0); p.y = (float)(v[1] * 0.5 + uin(rng) / 64.0); p.z = (float)(v[2] * 0.5 + uin(rng) / 64.0);
      scene.points.push_back(p);
    }

  // Rz(90 deg) + (3, -1.5, 7) and the cyclic axis permutation + (-2, 2.5, 1)
  Eigen::Matrix4d rz = Eigen::Matrix4d::Zero(), cyc = Eigen::Matrix4d::Zero();
  rz(0, 1) = -1; rz(1, 0) = 1; rz(2, 2) = 1; rz(3, 3) = 1; rz(0, 3) = 3; rz(1, 3) = -1.5; rz(2, 3) = 7;
  cyc(0, 2) = 1; cyc(1, 0) = 1; cyc(2, 1) = 1; cyc(3, 3) = 1; cyc(0, 3) = -2; cyc(1, 3) = 2.5; cyc(2, 3) = 1;

  Ndt a, direct;
  CHECK(a.lastStatus() == NDT_OK);
  a.setResolution(leaf);
  CHECK(a.mapTransform(rz) == 0 && a.lastStatus() == NDT_ERR_INVALID_ARG);       // no map
  fresh_map(a, leaf);
  CHECK(a.mapTransform(rz) == 0 && a.lastStatus() == NDT_OK);                    // an empty map: nothing, and no error
  a.mapAdd(scene);
  CHECK(a.lastStatus() == NDT_OK && a.mapInfo().n_voxels == 300);
  ndt_hip::MapState before, sa, sd;
  a.mapExportState(before);

  // mapTransform with an Eigen matrix, against a map fed the moved points
  CHECK(a.mapTransform(rz) == 300 && a.lastStatus() == NDT_OK);
  fresh_map(direct, leaf);
  direct.mapAdd(moved(scene, rz));
  a.mapExportState(sa);
  direct.mapExportState(sd);
  CHECK(sa.size() == 300 && same_state(sa, sd) && !same_state(sa, before));
  CHECK(a.mapInfo().n_points == (int64_t)scene.points.size() && a.mapInfo().n_adds == 1);

  // ... once more with a gtsam::Pose3 and with 16 column-major doubles: the same result
  Ndt g, raw;
  fresh_map(g, leaf);
  g.mapAdd(scene);
  CHECK(g.mapTransform(gtsam::Pose3(rz)) == 300 && g.lastStatus() == NDT_OK);
  ndt_hip::MapState sg;
  g.mapExportState(sg);
  CHECK(same_state(sg, sd));
  fresh_map(raw, leaf);
  raw.mapAdd(scene);
  const double* rz16 = rz.data();                                                // (column-major already)
  CHECK(raw.mapTransform(rz16) == 300);
  raw.mapExportState(sg);
  CHECK(same_state(sg, sd));

  // a second transform composes exactly on the lattice
  CHECK(a.mapTransform(gtsam::Pose3(cyc)) == 300);
  Ndt direct2;
  fresh_map(direct2, leaf);
  direct2.mapAdd(moved(moved(scene, rz), cyc));
  a.mapExportState(sa);
  direct2.mapExportState(sd);
  CHECK(same_state(sa, sd));

  // mapImportStatePosed: the saved state of a submap in its own frame, merged under its corrected pose (Eigen and gtsam)
  for (int form = 0; form < 2; ++form) {
    Ndt m;
    fresh_map(m, leaf);
    if (form == 0) m.mapImportStatePosed(before, cyc);
    else m.mapImportStatePosed(before, gtsam::Pose3(cyc));
    CHECK(m.lastStatus() == NDT_OK);
    Ndt d;
    fresh_map(d, leaf);
    d.mapAdd(moved(scene, cyc));
    ndt_hip::MapState sm;
    m.mapExportState(sm);
    d.mapExportState(sd);
    CHECK(same_state(sm, sd) && m.mapInfo().n_points == (int64_t)scene.points.size());
    // refusals: ragged vectors, another leaf size, a pose that is not finite -- each with the map as it was
    ndt_hip::MapState bad = before;
    bad.sums.pop_back();
    m.mapImportStatePosed(bad, cyc);
    CHECK(m.lastStatus() == NDT_ERR_INVALID_ARG);
    bad = before;
    bad.leaf = 1.0f;
    m.mapImportStatePosed(bad, cyc);
    CHECK(m.lastStatus() == NDT_ERR_INVALID_ARG);
    Eigen::Matrix4d nan = cyc;
    nan(1, 3) = std::nan("");
    m.mapImportStatePosed(before, nan);
    CHECK(m.lastStatus() == NDT_ERR_INVALID_ARG);
    CHECK(m.mapTransform(nan) == 0 && m.lastStatus() == NDT_ERR_INVALID_ARG);
    Eigen::Matrix4d far = Eigen::Matrix4d::Identity();
    far(0, 3) = 1048576.0;                                                       // 2^21 leaves
    CHECK(m.mapTransform(far) == 0 && m.lastStatus() == NDT_ERR_GRID_OVERFLOW);
    m.mapExportState(sm);
    CHECK(same_state(sm, sd));
  }

  std::printf("map repose: PASS (%zu points, %zu voxels)\n", scene.points.size(), before.size());
  return 0;
}
