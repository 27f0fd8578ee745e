// The C++ adapter's map-state surface (mapCrop / mapExportState / mapImportState) with PCL-typed clouds (API mocks,
// tests/cpp/mock), the way a driver that saves its map at shutdown, loads it at the next start and keeps a sliding
// window around the vehicle would use it.  The exported state is compared, bit for bit, with f32 / f64 sums made here
// per voxel in input order; a loaded map that goes on accumulating with one that never stopped.
// Needs a GPU.  Prints "map state: PASS" and returns 0 when everything agrees.
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
  float f[4] = {0, 0, 0, 0};
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};
using VoxelMapRef = std::map<std::array<int, 3>, Voxel>;   // key {k, j, i}: ascending as the export is

static bool same_state(const ndt_hip::MapState& a, const ndt_hip::MapState& b) {
  return a.leaf == b.leaf && a.ijk == b.ijk && a.counts == b.counts && a.sums.size() == b.sums.size() &&
         a.moments.size() == b.moments.size() &&
         (a.sums.empty() || std::memcmp(a.sums.data(), b.sums.data(), a.sums.size() * sizeof(float)) == 0) &&
         (a.moments.empty() || std::memcmp(a.moments.data(), b.moments.data(), a.moments.size() * sizeof(double)) == 0);
}

int main() {
  using Point = pcl::PointXYZ;
  using Cloud = pcl::PointCloud<Point>;
  const float leaf = 1.0f, inv_leaf = 1.0f / leaf;

  // three scans of a noisy slab, negative coordinates included: about 2000 voxels, up to a dozen points each
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> ux(-15.0f, 15.0f), uz(-1.0f, 1.5f);
  std::vector<Cloud> scans(3);
  for (auto& s : scans)
    for (int i = 0; i < 4000; ++i) {
      Point p{};
      p.x = ux(rng); p.y = ux(rng); p.z = uz(rng);
      s.points.push_back(p);
    }
  auto accumulate = [&](VoxelMapRef& want, const Cloud& c) {
    for (const auto& p : c.points) {
      const std::array<int, 3> key = {(int)std::floor(p.z * inv_leaf), (int)std::floor(p.y * inv_leaf),
                                      (int)std::floor(p.x * inv_leaf)};
      Voxel& v = want[key];
      const double a = p.x, b = p.y, d = p.z;
      ++v.count;
      v.f[0] += p.x; v.f[1] += p.y; v.f[2] += p.z;
      v.s[0] += a; v.s[1] += b; v.s[2] += d;
      v.s[3] += a * a; v.s[4] += a * b; v.s[5] += a * d;
      v.s[6] += b * b; v.s[7] += b * d; v.s[8] += d * d;
    }
  };
  auto equals = [&](const ndt_hip::MapState& st, const VoxelMapRef& want) {
    if (st.size() != want.size() || st.ijk.size() != 3 * st.size() || st.sums.size() != 4 * st.size() ||
        st.moments.size() != 9 * st.size())
      return false;
    size_t r = 0;
    for (const auto& kv : want) {
      if (st.ijk[3 * r] != kv.first[2] || st.ijk[3 * r + 1] != kv.first[1] || st.ijk[3 * r + 2] != kv.first[0]) return false;
      if (st.counts[r] != kv.second.count) return false;
      if (std::memcmp(&st.sums[4 * r], kv.second.f, sizeof(kv.second.f)) != 0) return false;
      if (std::memcmp(&st.moments[9 * r], kv.second.s, sizeof(kv.second.s)) != 0) return false;
      ++r;
    }
    return true;
  };

  pclomp::NormalDistributionsTransform<Point, Point> a;
  CHECK(a.lastStatus() == NDT_OK);
  a.setResolution(leaf);
  ndt_hip::MapState st;
  a.mapExportState(st);                          // no map
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG && st.size() == 0);
  const float lo[3] = {-5.0f, -5.0f, -1.0f}, hi[3] = {4.5f, 4.5f, 1.4f};
  a.mapCrop(lo, hi);
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG);
  a.mapReset(leaf);
  a.mapEnableMoments();
  a.mapExportState(st);                          // an empty map: nothing, and no error
  CHECK(a.lastStatus() == NDT_OK && st.size() == 0 && st.leaf == leaf);
  a.mapAdd(scans[0]);
  a.mapAdd(scans[1]);
  CHECK(a.lastStatus() == NDT_OK);

  // the export: sizes, order and every bit of the float sums and of the moments
  VoxelMapRef want01;
  accumulate(want01, scans[0]);
  accumulate(want01, scans[1]);
  a.mapExportState(st);
  CHECK(a.lastStatus() == NDT_OK && st.leaf == leaf && !st.with_intensity);
  CHECK(equals(st, want01));
  CHECK((int64_t)st.size() == a.mapInfo().n_voxels);

  // save -> load on a second engine; both go on with the third scan and agree with the map that never stopped
  pclomp::NormalDistributionsTransform<Point, Point> b;
  b.mapReset(leaf);
  b.mapEnableMoments();
  b.mapImportState(st);
  CHECK(b.lastStatus() == NDT_OK);
  CHECK(b.mapInfo().n_voxels == a.mapInfo().n_voxels && b.mapInfo().n_points == a.mapInfo().n_points);
  a.mapAdd(scans[2]);
  b.mapAdd(scans[2]);
  VoxelMapRef want012 = want01;
  accumulate(want012, scans[2]);
  ndt_hip::MapState sa, sb;
  a.mapExportState(sa);
  b.mapExportState(sb);
  CHECK(a.lastStatus() == NDT_OK && b.lastStatus() == NDT_OK);
  CHECK(equals(sa, want012) && same_state(sa, sb));

  // refusals: a state of another leaf size, a state without moments for a map that keeps them, ragged vectors
  ndt_hip::MapState bad = st;
  bad.leaf = 0.5f;
  b.mapImportState(bad);
  CHECK(b.lastStatus() == NDT_ERR_INVALID_ARG);
  bad = st;
  bad.moments.clear();
  b.mapImportState(bad);
  CHECK(b.lastStatus() == NDT_ERR_INVALID_ARG);
  bad = st;
  bad.sums.pop_back();
  b.mapImportState(bad);
  CHECK(b.lastStatus() == NDT_ERR_INVALID_ARG);
  b.mapExportState(sb);
  CHECK(same_state(sa, sb));                     // ... each with the map as it was

  // the box export and the crop: both ends included, in the voxel's own f32 floor
  VoxelMapRef inside, outside;
  for (const auto& kv : want012) {
    bool in = true;
    for (int ax = 0; ax < 3; ++ax) {
      const int v = kv.first[2 - ax];
      in = in && v >= (int)std::floor(lo[ax] * inv_leaf) && v <= (int)std::floor(hi[ax] * inv_leaf);
    }
    (in ? inside : outside)[kv.first] = kv.second;
  }
  CHECK(inside.size() > 50 && outside.size() > 50);
  ndt_hip::MapState boxed;
  a.mapExportState(boxed, lo, hi);
  CHECK(a.lastStatus() == NDT_OK && equals(boxed, inside));
  a.mapExportState(boxed, lo, nullptr);
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG && boxed.size() == 0);
  CHECK(a.mapCrop(lo, hi) == (int64_t)outside.size() && a.lastStatus() == NDT_OK);
  a.mapExportState(sa);
  CHECK(equals(sa, inside) && a.mapInfo().n_voxels == (int64_t)inside.size());
  CHECK(a.mapCrop(lo, hi) == 0 && a.lastStatus() == NDT_OK);          // nothing left to remove
  CHECK(b.mapCrop(lo, hi, true) == (int64_t)inside.size() && b.lastStatus() == NDT_OK);
  b.mapExportState(sb);
  CHECK(equals(sb, outside));

  // merge: the two halves back into one map -- no voxel is shared, so every record arrives bit for bit
  a.mapImportState(sb);
  CHECK(a.lastStatus() == NDT_OK);
  a.mapExportState(sa);
  CHECK(equals(sa, want012));
  // ... and a target made from the merged map's moments has the leaves of one made from the points
  auto all = std::make_shared<Cloud>();
  for (const auto& s : scans) all->points.insert(all->points.end(), s.points.begin(), s.points.end());
  pclomp::NormalDistributionsTransform<Point, Point> ref;
  ref.setResolution(leaf);
  ref.setInputTarget(all);
  a.setInputTargetFromMapMoments();
  CHECK(a.lastStatus() == NDT_OK && ref.lastStatus() == NDT_OK);
  const auto got = a.getTargetCells().getLeaves(), want_leaves = ref.getTargetCells().getLeaves();
  CHECK(!got.empty() && got.size() == want_leaves.size());
  for (size_t i = 0; i < got.size(); ++i)
    CHECK(got[i].first == want_leaves[i].first && got[i].second.getPointCount() == want_leaves[i].second.getPointCount());

  std::printf("map state: PASS (%zu voxels, %zu inside the box, %zu leaves)\n", want012.size(), inside.size(), got.size());
  return 0;
}
