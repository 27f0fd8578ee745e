// The C++ adapter's level surface (mapLevelInfo, mapExportStateLevel, setInputTargetFromMapLevel, mapCoarsen,
// mapLevelsDrop, alignMapLevels) with PCL-typed clouds and Eigen poses (API mocks, tests/cpp/mock), the way a driver that
// closes a loop against its own map would use it: a 0.5 m map, its 1 m and 2 m levels as coarse targets, a scan that
// starts 0.8 m off.  The level's records are compared, bit for bit, with sums made here from the map's own records in
// ascending child order; the level target with the target of a second map that imported those records.
// Needs a GPU.  Prints "map levels: PASS" and returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/ndt_omp.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <vector>

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                         \
    }                                                                   \
  } while (0)

using Point = pcl::PointXYZ;
using Cloud = pcl::PointCloud<Point>;
using Ndt = pclomp::NormalDistributionsTransform<Point, Point>;

// wavy ground and two walls on 30 m x 30 m, seen from a frame shifted by (dx, dy)
static std::shared_ptr<Cloud> sample(int n, unsigned seed, double dx, double dy) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> u(-15.0, 15.0), h(0.0, 4.0), noise(-0.02, 0.02);
  auto out = std::make_shared<Cloud>();
  for (int i = 0; i < n; ++i) {
    double p[3];
    const int kind = i % 4;
    if (kind < 2) { p[0] = u(rng); p[1] = u(rng); p[2] = 0.4 * std::sin(p[0] / 3.0) * std::cos(p[1] / 4.0); }
    else if (kind == 2) { p[0] = 6.4; p[1] = u(rng); p[2] = h(rng); }
    else { p[0] = u(rng); p[1] = -7.3; p[2] = h(rng); }
    Point q{};
    q.x = (float)(p[0] + noise(rng) - dx); q.y = (float)(p[1] + noise(rng) - dy); q.z = (float)(p[2] + noise(rng));
    out->points.push_back(q);
  }
  return out;
}

struct Sums {
  long long count = 0;
  float s[4] = {0, 0, 0, 0};
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};

int main() {
  const float leaf = 0.5f;
  Ndt a;
  CHECK(a.lastStatus() == NDT_OK);
  a.setResolution(leaf);
  a.setMaximumIterations(35);
  a.setTransformationEpsilon(1e-4);
  a.setStepSize(0.1);
  a.mapLevelInfo(1);
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG);     // no map
  a.mapReset(leaf);
  a.mapEnableMoments();
  a.mapAdd(*sample(30000, 3, 0.0, 0.0));
  CHECK(a.lastStatus() == NDT_OK);

  // level 1 against the rule, from the map's own records (ascending (k, j, i): so are the children of every parent)
  ndt_hip::MapState fine, lv;
  a.mapExportState(fine);
  CHECK(a.lastStatus() == NDT_OK && fine.size() > 1000);
  std::map<std::array<int, 3>, Sums> want;   // key {k, j, i} of the parent
  for (size_t r = 0; r < fine.size(); ++r) {
    Sums& w = want[{fine.ijk[3 * r + 2] >> 1, fine.ijk[3 * r + 1] >> 1, fine.ijk[3 * r] >> 1}];
    w.count += fine.counts[r];
    for (int f = 0; f < 3; ++f) w.s[f] += fine.sums[4 * r + f];
    for (int f = 0; f < 9; ++f) w.m[f] += fine.moments[9 * r + f];
  }
  a.mapExportStateLevel(1, lv);
  CHECK(a.lastStatus() == NDT_OK && lv.size() == want.size() && lv.leaf == 1.0f && lv.moments.size() == 9 * lv.size());
  size_t r = 0;
  for (const auto& kv : want) {
    CHECK(lv.ijk[3 * r] == kv.first[2] && lv.ijk[3 * r + 1] == kv.first[1] && lv.ijk[3 * r + 2] == kv.first[0]);
    CHECK(lv.counts[r] == kv.second.count);
    CHECK(std::memcmp(&lv.sums[4 * r], kv.second.s, sizeof(kv.second.s)) == 0);
    CHECK(std::memcmp(&lv.moments[9 * r], kv.second.m, sizeof(kv.second.m)) == 0);
    ++r;
  }
  const ndt_map_info li = a.mapLevelInfo(1), mi = a.mapInfo();
  CHECK(a.lastStatus() == NDT_OK && li.leaf == 1.0f && (size_t)li.n_voxels == lv.size() && li.n_points == mi.n_points);
  CHECK(a.mapLevelInfo(0).n_voxels == mi.n_voxels && a.mapLevelInfo(0).leaf == leaf);
  a.mapLevelInfo(7);
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG);
  const float lo[3] = {-5.0f, -5.0f, -1.0f}, hi[3] = {4.5f, 4.5f, 1.4f};
  ndt_hip::MapState boxed;
  a.mapExportStateLevel(1, boxed, lo, hi);
  CHECK(a.lastStatus() == NDT_OK && boxed.size() > 0 && boxed.size() < lv.size());

  // the level as the target: what a map of leaf 1.0 that imported the level's records builds from its moments
  a.setInputTargetFromMapLevel(1);
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG);     // the resolution is the map's leaf, not the level's
  a.setResolution(1.0f);
  a.setInputTargetFromMapLevel(1);
  CHECK(a.lastStatus() == NDT_OK);
  Ndt b;
  b.setResolution(1.0f);
  b.mapReset(1.0f);
  b.mapEnableMoments();
  b.mapImportState(lv);
  b.setInputTargetFromMapMoments();
  CHECK(b.lastStatus() == NDT_OK);
  const auto got = a.getTargetCells().getLeaves(), ref = b.getTargetCells().getLeaves();
  CHECK(!got.empty() && got.size() == ref.size());
  for (size_t i = 0; i < got.size(); ++i) {
    CHECK(got[i].first == ref[i].first && got[i].second.getPointCount() == ref[i].second.getPointCount());
    for (int f = 0; f < 3; ++f) CHECK(got[i].second.d.mean[f] == ref[i].second.d.mean[f]);
  }
  a.setResolution(leaf);

  // coarse to fine from 0.8 m off: one result per step, the last one at the truth; a bad level stops the sequence
  a.setInputSource(sample(6000, 9, 0.8, -0.3));
  const std::vector<ndt_map_level_step> steps = {{2, 0, 0.0}, {1, 0, 0.0}, {0, 0, 0.0}};
  const auto res = a.alignMapLevels(steps, Eigen::Matrix4f::Identity());
  CHECK(a.lastStatus() == NDT_OK && res.size() == 3);
  const float* T = res[2].final_transformation;
  std::printf("levels [2, 1, 0]: t = (%.4f, %.4f, %.4f) after %d + %d + %d iterations\n", T[12], T[13], T[14], res[0].iterations,
              res[1].iterations, res[2].iterations);
  CHECK(std::fabs(T[12] - 0.8f) < 0.05f && std::fabs(T[13] + 0.3f) < 0.05f && std::fabs(T[14]) < 0.05f);
  CHECK(a.getResolution() == leaf);
  const std::vector<ndt_map_level_step> bad = {{2, 0, 0.0}, {7, 0, 0.0}, {0, 0, 0.0}};
  const auto part = a.alignMapLevels(bad, Eigen::Matrix4f::Identity());
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG && part.size() == 1);
  CHECK(a.alignMapLevels({}, Eigen::Matrix4f::Identity()).empty() && a.lastStatus() == NDT_ERR_INVALID_ARG);

  // drop and coarsen
  a.mapLevelsDrop();
  CHECK(a.lastStatus() == NDT_OK);
  a.mapCoarsen(1);
  CHECK(a.lastStatus() == NDT_OK && a.mapInfo().leaf == 1.0f && (size_t)a.mapInfo().n_voxels == lv.size());
  ndt_hip::MapState after;
  a.mapExportState(after);
  CHECK(after.ijk == lv.ijk && after.counts == lv.counts && after.sums == lv.sums && after.moments == lv.moments);
  std::printf("map levels: PASS (%zu voxels, %zu at level 1, %zu in the box, %zu leaves)\n", fine.size(), lv.size(), boxed.size(),
              got.size());
  return 0;
}
