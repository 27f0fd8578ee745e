// The C++ adapter's moments surface (mapEnableMoments / mapHasMoments / mapExportMoments /
// setInputTargetFromMapMoments) with PCL-typed clouds (API mocks, tests/cpp/mock), the way a driver that localises against
// the map it accumulates would use it.  The moments are compared, bit for bit, with f64 sums made here per voxel in
// input order; the target with the one setInputTarget builds from the concatenation.
// Needs a GPU.  Prints "map target: PASS" and returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/ndt_omp.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                         \
    }                                                                   \
  } while (0)

struct Voxel {
  int count = 0;
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};

int main() {
  using Point = pcl::PointXYZ;
  using Cloud = pcl::PointCloud<Point>;
  pclomp::NormalDistributionsTransform<Point, Point> ndt;
  CHECK(ndt.lastStatus() == NDT_OK);
  const float leaf = 1.0f, inv_leaf = 1.0f / leaf;
  ndt.setResolution(leaf);

  // three scans of a noisy slab, negative coordinates included: about 2000 voxels, up to a dozen points each
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> ux(-15.0f, 15.0f), uz(-1.0f, 1.5f);
  std::vector<Cloud> scans(3);
  auto all = std::make_shared<Cloud>();
  for (auto& s : scans)
    for (int i = 0; i < 4000; ++i) {
      Point p{};
      p.x = ux(rng); p.y = ux(rng); p.z = uz(rng);
      s.points.push_back(p);
      all->points.push_back(p);
    }

  // the yardstick: per voxel, in ascending (k, j, i), the nine f64 sums in input order
  std::map<std::array<int, 3>, Voxel> want;   // key {k, j, i}
  for (const auto& p : all->points) {
    const std::array<int, 3> key = {(int)std::floor(p.z * inv_leaf), (int)std::floor(p.y * inv_leaf),
                                    (int)std::floor(p.x * inv_leaf)};
    Voxel& v = want[key];
    const double a = p.x, b = p.y, c = p.z;
    ++v.count;
    v.s[0] += a; v.s[1] += b; v.s[2] += c;
    v.s[3] += a * a; v.s[4] += a * b; v.s[5] += a * c;
    v.s[6] += b * b; v.s[7] += b * c; v.s[8] += c * c;
  }

  std::vector<int32_t> ijk, counts;
  std::vector<double> sums;
  // state: no map, a map without moments, a map with points
  CHECK(!ndt.mapHasMoments());
  ndt.mapEnableMoments();
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  ndt.mapReset(leaf);
  CHECK(ndt.lastStatus() == NDT_OK && !ndt.mapHasMoments());
  ndt.mapExportMoments(ijk, counts, sums);
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG && ijk.empty() && counts.empty() && sums.empty());
  ndt.setInputTargetFromMapMoments();
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  ndt.mapAdd(scans[0]);
  ndt.mapEnableMoments();
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG && !ndt.mapHasMoments());

  ndt.mapReset(leaf);
  ndt.mapEnableMoments();
  CHECK(ndt.lastStatus() == NDT_OK && ndt.mapHasMoments());
  ndt.mapEnableMoments();
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG && ndt.mapHasMoments());
  ndt.mapExportMoments(ijk, counts, sums);       // an empty map: nothing, and no error
  CHECK(ndt.lastStatus() == NDT_OK && ijk.empty() && counts.empty() && sums.empty());
  for (const auto& s : scans) {
    ndt.mapAdd(s);
    CHECK(ndt.lastStatus() == NDT_OK);
  }

  // the export: sizes, order and every bit
  ndt.mapExportMoments(ijk, counts, sums);
  CHECK(ndt.lastStatus() == NDT_OK);
  const size_t m = counts.size();
  CHECK(m == want.size() && ijk.size() == 3 * m && sums.size() == 9 * m);
  CHECK((int64_t)m == ndt.mapInfo().n_voxels);
  size_t r = 0, n_big = 0;
  long total = 0;
  for (const auto& kv : want) {
    CHECK(ijk[3 * r] == kv.first[2] && ijk[3 * r + 1] == kv.first[1] && ijk[3 * r + 2] == kv.first[0]);
    CHECK(counts[r] == kv.second.count);
    CHECK(std::memcmp(&sums[9 * r], kv.second.s, sizeof(kv.second.s)) == 0);
    total += counts[r];
    n_big += kv.second.count >= 8 ? 1 : 0;
    ++r;
  }
  CHECK(total == (long)all->points.size() && n_big > 0 && n_big < m);
  std::vector<int32_t> ijk8, counts8;
  std::vector<double> sums8;
  ndt.mapExportMoments(ijk8, counts8, sums8, 8);
  CHECK(ndt.lastStatus() == NDT_OK && counts8.size() == n_big && ijk8.size() == 3 * n_big && sums8.size() == 9 * n_big);
  for (int c : counts8) CHECK(c >= 8);

  // the target from the moments: the leaves setInputTarget builds from the concatenation
  pclomp::NormalDistributionsTransform<Point, Point> ref;
  ref.setResolution(leaf);
  ref.setInputTarget(all);
  CHECK(ref.lastStatus() == NDT_OK);
  const auto want_leaves = ref.getTargetCells().getLeaves();
  ndt.setInputTargetFromMapMoments();
  CHECK(ndt.lastStatus() == NDT_OK);
  const auto got = ndt.getTargetCells().getLeaves();
  CHECK(!got.empty() && got.size() == want_leaves.size());
  for (size_t i = 0; i < got.size(); ++i) {
    CHECK(got[i].first == want_leaves[i].first);
    CHECK(got[i].second.getPointCount() == want_leaves[i].second.getPointCount());
    for (int a = 0; a < 3; ++a)
      CHECK(std::fabs(got[i].second.d.mean[a] - want_leaves[i].second.d.mean[a]) <= 1e-12 * std::fabs(want_leaves[i].second.d.mean[a]));
  }

  // a box (both ends included, in the voxel's own f32 floor): fewer leaves, every one of them inside; an empty box and a
  // leaf size that is not the resolution are refused with the target as it was
  const float lo[3] = {-5.0f, -5.0f, -1.0f}, hi[3] = {4.5f, 4.5f, 1.4f};
  ndt.setInputTargetFromMapMoments(lo, hi);
  CHECK(ndt.lastStatus() == NDT_OK);
  const auto boxed = ndt.getTargetCells().getLeaves();
  CHECK(!boxed.empty() && boxed.size() < got.size());
  for (const auto& e : boxed)
    for (int a = 0; a < 3; ++a)
      CHECK(e.second.d.mean[a] >= std::floor(lo[a]) && e.second.d.mean[a] < std::floor(hi[a]) + 1.0);
  const float far_lo[3] = {500.0f, 500.0f, 0.0f}, far_hi[3] = {510.0f, 510.0f, 5.0f};
  ndt.setInputTargetFromMapMoments(far_lo, far_hi);
  CHECK(ndt.lastStatus() == NDT_ERR_NO_TARGET);
  CHECK(ndt.getTargetCells().getLeaves().size() == boxed.size());
  ndt.setInputTargetFromMapMoments(lo, nullptr);
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  ndt.setResolution(2.0f);     // the grid is dropped (nothing was retained) ...
  ndt.setInputTargetFromMapMoments();
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  ndt.setResolution(leaf);     // ... and made again from the map
  ndt.setInputTargetFromMapMoments();
  CHECK(ndt.lastStatus() == NDT_OK && ndt.getTargetCells().getLeaves().size() == got.size());

  ndt.mapReset(leaf);
  CHECK(ndt.lastStatus() == NDT_OK && !ndt.mapHasMoments());
  std::printf("map target: PASS (%zu voxels, %zu with 8 points or more, %zu leaves, %zu in the box)\n", m, n_big, got.size(),
              boxed.size());
  return 0;
}
