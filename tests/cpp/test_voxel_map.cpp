// The C++ adapter's voxel-map surface (mapReset / mapAdd / mapExport / setInputTargetFromMap) with PCL-typed clouds
// (API mocks, tests/cpp/mock), written the way run/pipeline_ins_map_distribution.cpp's cumm_thread would use it.
// Needs a GPU.  Prints "voxel map: PASS" and returns 0 when everything agrees bit for bit.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/ndt_omp.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                         \
    }                                                                   \
  } while (0)

template <class P>
static bool same_xyz(const P& a, const P& b) {
  return std::memcmp(&a.x, &b.x, 3 * sizeof(float)) == 0;
}

int main() {
  using PointI = pcl::PointXYZI;
  using CloudI = pcl::PointCloud<PointI>;
  pclomp::NormalDistributionsTransform<PointI, PointI> ndt;
  CHECK(ndt.lastStatus() == NDT_OK);

  // three scans of a noisy box, negative coordinates included
  std::mt19937 rng(5);
  std::uniform_real_distribution<float> ux(-20.0f, 20.0f), uz(-2.0f, 3.0f), ui(0.0f, 255.0f);
  std::vector<CloudI> scans(3);
  CloudI all;
  for (auto& s : scans)
    for (int i = 0; i < 3000; ++i) {
      PointI p{};
      p.x = ux(rng); p.y = ux(rng); p.z = uz(rng); p.intensity = ui(rng);
      s.points.push_back(p);
      all.points.push_back(p);
    }
  const float leaf = 0.5f;

  // without a pose, intensity picked up from the point type: equal to voxelDownsample of the concatenation
  CloudI want;
  ndt.voxelDownsample(all, leaf, want);
  CHECK(ndt.lastStatus() == NDT_OK && !want.points.empty());
  ndt.mapExport(want, 1);                       // before mapReset: refused
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG && want.points.empty());
  ndt.voxelDownsample(all, leaf, want);
  ndt.mapReset(leaf, /*with_intensity=*/true);
  CHECK(ndt.lastStatus() == NDT_OK);
  for (const auto& s : scans) {
    ndt.mapAdd(s);
    CHECK(ndt.lastStatus() == NDT_OK);
  }
  CloudI got;
  std::vector<int32_t> counts;
  ndt.mapExport(got, 1, &counts);
  CHECK(ndt.lastStatus() == NDT_OK);
  CHECK(got.points.size() == want.points.size() && counts.size() == got.points.size());
  long total = 0;
  for (size_t i = 0; i < got.points.size(); ++i) {
    CHECK(same_xyz(got.points[i], want.points[i]));
    CHECK(std::memcmp(&got.points[i].intensity, &want.points[i].intensity, sizeof(float)) == 0);
    total += counts[i];
  }
  CHECK(total == (long)all.points.size());
  const ndt_map_info mi = ndt.mapInfo();
  CHECK(ndt.lastStatus() == NDT_OK && mi.n_voxels == (int64_t)got.points.size() && mi.n_points == (int64_t)all.points.size());
  CHECK(mi.with_intensity == 1 && mi.n_adds == 3 && mi.capacity >= 2 * mi.n_voxels);

  // a map with intensity refuses a cloud whose point type has none
  pcl::PointCloud<pcl::PointXYZ> bare;
  bare.points.resize(10);
  ndt.mapAdd(bare);
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG);

  // with a pose (column-major 4x4 doubles): equal to the map of the clouds moved on the host with the same arithmetic
  const double c = 0.8, s = 0.6;
  const double pose[16] = {c, s, 0, 0, -s, c, 0, 0, 0, 0, 1, 0, 12.5, -7.25, 0.75, 1};
  pcl::PointCloud<pcl::PointXYZ> moved_all;
  std::vector<pcl::PointCloud<pcl::PointXYZ>> plain(3);
  for (size_t k = 0; k < scans.size(); ++k)
    for (const auto& p : scans[k].points) {
      pcl::PointXYZ q{}, m{};
      q.x = p.x; q.y = p.y; q.z = p.z;
      plain[k].points.push_back(q);
      const double a = p.x, b = p.y, d = p.z;
      m.x = (float)(pose[0] * a + pose[4] * b + pose[8] * d + pose[12]);
      m.y = (float)(pose[1] * a + pose[5] * b + pose[9] * d + pose[13]);
      m.z = (float)(pose[2] * a + pose[6] * b + pose[10] * d + pose[14]);
      moved_all.points.push_back(m);
    }
  pcl::PointCloud<pcl::PointXYZ> want3, got3;
  ndt.voxelDownsample(moved_all, leaf, want3);
  CHECK(ndt.lastStatus() == NDT_OK);
  ndt.mapReset(leaf);
  for (const auto& s3 : plain) {
    ndt.mapAdd(s3, pose);
    CHECK(ndt.lastStatus() == NDT_OK);
  }
  ndt.mapExport(got3);
  CHECK(ndt.lastStatus() == NDT_OK && got3.points.size() == want3.points.size());
  for (size_t i = 0; i < got3.points.size(); ++i) CHECK(same_xyz(got3.points[i], want3.points[i]));

  // the map as the target: the leaves of the exported cloud
  ndt.setResolution(2.0f);
  ndt.setInputTargetFromMap(1);
  CHECK(ndt.lastStatus() == NDT_OK);
  const size_t n_map = ndt.getTargetCells().getLeaves().size();
  auto tgt = std::make_shared<pcl::PointCloud<PointI>>();
  for (const auto& p : got3.points) {
    PointI q{};
    q.x = p.x; q.y = p.y; q.z = p.z;
    tgt->points.push_back(q);
  }
  ndt.setInputTarget(tgt);
  CHECK(ndt.lastStatus() == NDT_OK);
  CHECK(n_map > 0 && ndt.getTargetCells().getLeaves().size() == n_map);

  ndt.mapClear();
  CHECK(ndt.lastStatus() == NDT_OK);
  ndt.mapAdd(plain[0]);
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  std::printf("voxel map: PASS (%zu voxels with intensity, %zu under a pose, %zu leaves)\n", got.points.size(),
              got3.points.size(), n_map);
  return 0;
}
