// The C++ adapter's per-point scoring surface against the C calls it wraps: scorePoints, the recalled tier4 name
// calculateNearestVoxelScoreEachPoint through the pclomp compat header, nearestVoxelScoreEachPoint and filterSource.
// Needs a GPU.  Prints "point scores: OK" and returns 0 when everything agrees.
#include <pclomp/ndt_omp.h>

#include <cmath>
#include <cstdio>
#include <cstring>
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

using Point = ndt_hip::PointXYZI;
using Cloud = ndt_hip::PointCloud<Point>;
using Ndt = pclomp::NormalDistributionsTransform<Point, Point>;

int main() {
  // two noisy planes, the source a shifted subset
  std::mt19937 rng(17);
  std::normal_distribution<float> noise(0.0f, 0.02f);
  auto target = std::make_shared<Cloud>();
  auto source = std::make_shared<Cloud>();
  for (int i = 0; i < 120; ++i)
    for (int j = 0; j < 120; ++j) {
      Point a{}, b{};
      a.x = 0.1f * i; a.y = 0.1f * j; a.z = noise(rng);
      b.x = 0.1f * i; b.y = noise(rng); b.z = 0.1f * j;
      target->points.push_back(a);
      target->points.push_back(b);
      if ((i + j) % 3 == 0) {
        a.x += 0.05f; b.z += 0.03f;
        source->points.push_back(a);
        source->points.push_back(b);
      }
    }
  Point far{};
  far.x = 500.0f;                       // a point the map does not explain
  source->points.push_back(far);

  Ndt ndt;
  CHECK(ndt.lastStatus() == NDT_OK);
  ndt.setResolution(1.0f);
  ndt.setNeighborhoodSearchMethod(pclomp::DIRECT7);
  ndt.setInputTarget(target);
  ndt.setInputSource(source);
  const size_t n = source->points.size();
  ndt_hip::Matrix4f T = ndt_hip::identity4f();
  T(0, 3) = 0.02f;
  float a[16];
  ndt_hip::detail::to_colmajor(T, 4, 4, a);

  // the C calls
  std::vector<double> score(n), nvs(n);
  std::vector<int32_t> nn(n);
  std::vector<int64_t> bv(n);
  CHECK(ndt_source_size(ndt.handle()) == (int64_t)n);
  CHECK(ndt_score_points(ndt.handle(), a, score.data(), nvs.data(), nn.data(), bv.data(), n) == NDT_OK);
  std::vector<float> moved(3 * n);
  CHECK(ndt_transform_source(ndt.handle(), a, moved.data(), n) == NDT_OK);
  CHECK(nn[n - 1] == 0 && nvs[n - 1] == 0.0 && bv[n - 1] == -1);

  // scorePoints
  const auto ps = ndt.scorePoints(T);
  CHECK(ndt.lastStatus() == NDT_OK && ps.size() == n);
  CHECK(std::memcmp(ps.score.data(), score.data(), n * sizeof(double)) == 0);
  CHECK(std::memcmp(ps.nearest_voxel_score.data(), nvs.data(), n * sizeof(double)) == 0);
  CHECK(ps.n_neighbors == nn && ps.best_voxel == bv);

  // nearestVoxelScoreEachPoint: the transformed source, intensity = nearest_voxel_score
  const Cloud each = ndt.nearestVoxelScoreEachPoint(T);
  CHECK(ndt.lastStatus() == NDT_OK && each.points.size() == n);
  size_t explained = 0;
  for (size_t i = 0; i < n; ++i) {
    CHECK(each.points[i].x == moved[3 * i] && each.points[i].y == moved[3 * i + 1] && each.points[i].z == moved[3 * i + 2]);
    CHECK(each.points[i].intensity == (float)nvs[i]);
    explained += nvs[i] > 0.0;
  }
  CHECK(explained > n / 2);

  // filterSource against the C call and against the per-point values
  const double thr = 0.5;
  std::vector<float> fx(3 * n);
  std::vector<int32_t> fi(n);
  size_t m = 0;
  for (int below = 0; below < 2; ++below) {
    CHECK(ndt_filter_source(ndt.handle(), a, thr, below, fx.data(), fi.data(), n, &m) == NDT_OK);
    std::vector<int32_t> idx;
    const Cloud kept = ndt.filterSource(T, thr, below != 0, &idx);
    CHECK(ndt.lastStatus() == NDT_OK && kept.points.size() == m && idx.size() == m);
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {
      if ((below ? nvs[i] < thr : nvs[i] >= thr)) {
        CHECK(k < m && idx[k] == (int32_t)i && fi[k] == (int32_t)i);
        CHECK(kept.points[k].x == source->points[i].x && kept.points[k].y == source->points[i].y &&
              kept.points[k].z == source->points[i].z);
        CHECK(fx[3 * k] == source->points[i].x);
        ++k;
      }
    }
    CHECK(k == m);
  }

  // the recalled tier4 call, through the compat name: the cloud is taken as already transformed
  Cloud pre;
  pre.points.resize(n);
  for (size_t i = 0; i < n; ++i) { pre.points[i].x = moved[3 * i]; pre.points[i].y = moved[3 * i + 1]; pre.points[i].z = moved[3 * i + 2]; }
  const Cloud t4 = ndt.calculateNearestVoxelScoreEachPoint(pre);
  CHECK(ndt.lastStatus() == NDT_OK && t4.points.size() == n);
  for (size_t i = 0; i < n; ++i) {
    CHECK(t4.points[i].x == moved[3 * i] && t4.points[i].y == moved[3 * i + 1] && t4.points[i].z == moved[3 * i + 2]);
    CHECK(t4.points[i].intensity == (float)nvs[i]);   // the same f32 points in the same voxels: the same pair scores
  }
  std::printf("point scores: OK (%zu points, %zu explained)\n", n, explained);
  return 0;
}
