// The C++ adapter's free-space carving (mapCarve / mapCarveDevice / mapCarveKeyframe) with PCL-typed clouds (API mocks,
// tests/cpp/mock), the way a mapping driver would use it: every keyframe scan is added to the map, and the map is then
// carved with the same scan so that what the scan looks through goes.  The expected survivors come from the rules of
// ndt_hip.h written out here one ray at a time (Amanatides-Woo in f64, ties to the lowest axis).
// Needs a GPU.  Prints "map carve: PASS" and returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/ndt_omp.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                         \
    }                                                                   \
  } while (0)

using Key = std::array<int, 3>;   // {k, j, i}: ascending as the export is
struct Mark {
  long misses = 0;
  bool hit = false;
};

// the marks of one ray (rules 1, 3 and 4; no pose, every point finite and in range); returns the ray's share of n_steps
static long mark_ray(const float o[3], const float p[3], float inv_leaf, int keep_last, int max_steps, std::map<Key, Mark>& marks) {
  double gs[3], ge[3], tmax[3], tdelta[3];
  int v[3], ve[3], step[3];
  long L = 0;
  for (int a = 0; a < 3; ++a) {
    gs[a] = (double)(o[a] * inv_leaf);
    ge[a] = (double)(p[a] * inv_leaf);
    v[a] = (int)std::floor(gs[a]);
    ve[a] = (int)std::floor(ge[a]);
    L += std::abs(ve[a] - v[a]);
    tmax[a] = std::numeric_limits<double>::infinity();
    tdelta[a] = 0.0;
    step[a] = ve[a] > v[a] ? 1 : -1;
    if (ve[a] != v[a]) {
      const double d = ge[a] - gs[a];
      tdelta[a] = 1.0 / std::fabs(d);
      tmax[a] = ((double)(v[a] + (step[a] > 0 ? 1 : 0)) - gs[a]) / d;
    }
  }
  const long bound = std::min<long>(L - 1 - keep_last, max_steps);
  for (long i = 1; i <= bound; ++i) {
    const int a = (tmax[0] <= tmax[1] && tmax[0] <= tmax[2]) ? 0 : (tmax[1] <= tmax[2] ? 1 : 2);
    v[a] += step[a];
    tmax[a] = v[a] == ve[a] ? std::numeric_limits<double>::infinity() : tmax[a] + tdelta[a];
    ++marks[Key{v[2], v[1], v[0]}].misses;
  }
  marks[Key{ve[2], ve[1], ve[0]}].hit = true;
  return std::max<long>(bound, 0);
}

int main() {
  using Point = pcl::PointXYZ;
  using Cloud = pcl::PointCloud<Point>;
  const float leaf = 0.5f, inv_leaf = 1.0f / leaf;
  const float origin[3] = {0.2f, 0.1f, 0.4f};

  // a wall at x = 10 seen through a fan of 61 x 21 rays, and a parked box (a slab of points around x = 5) in front of it
  Cloud wall, box;
  for (int a = -30; a <= 30; ++a)
    for (int e = -10; e <= 10; ++e) {
      const double az = a * 0.0123, el = e * 0.0171;
      const double t = (10.0 - origin[0]) / (std::cos(el) * std::cos(az));
      Point p{};
      p.x = (float)(origin[0] + t * std::cos(el) * std::cos(az));
      p.y = (float)(origin[1] + t * std::cos(el) * std::sin(az));
      p.z = (float)(origin[2] + t * std::sin(el));
      wall.points.push_back(p);
    }
  for (int i = 0; i < 12; ++i)
    for (int j = 0; j < 12; ++j) {
      Point p{};
      p.x = 5.05f + 0.07f * (float)(i % 3); p.y = -0.9f + 0.15f * (float)i; p.z = -0.4f + 0.12f * (float)j;
      box.points.push_back(p);
    }

  pclomp::NormalDistributionsTransform<Point, Point> a;
  CHECK(a.lastStatus() == NDT_OK);
  a.setResolution(leaf);
  ndt_map_carve_result r = a.mapCarve(wall, origin);                 // no map
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG && r.n_rays == 0);
  a.mapReset(leaf);
  a.mapEnableMoments();
  a.mapAdd(wall);
  a.mapAdd(box);
  CHECK(a.lastStatus() == NDT_OK);
  ndt_hip::MapState before;
  a.mapExportState(before);
  CHECK(a.lastStatus() == NDT_OK && before.size() > 100);

  // what the rules say
  ndt_map_carve_params prm;
  ndt_map_carve_default_params(&prm);
  CHECK(prm.min_misses == 2 && prm.keep_last == 1 && prm.max_steps == 4096 && prm.protect_min_count == 0 && prm.dry_run == 0);
  std::map<Key, Mark> marks;
  long steps = 0;
  for (const auto& p : wall.points) {
    const float q[3] = {p.x, p.y, p.z};
    steps += mark_ray(origin, q, inv_leaf, prm.keep_last, prm.max_steps, marks);
  }
  std::vector<char> keep(before.size(), 1);
  int64_t removed = 0, pts_removed = 0, crossed = 0, hit = 0;
  for (size_t i = 0; i < before.size(); ++i) {
    const auto it = marks.find(Key{before.ijk[3 * i + 2], before.ijk[3 * i + 1], before.ijk[3 * i]});
    if (it == marks.end()) continue;
    crossed += it->second.misses > 0;
    hit += it->second.hit;
    if (it->second.misses >= prm.min_misses && !it->second.hit) {
      keep[i] = 0;
      ++removed;
      pts_removed += before.counts[i];
    }
  }
  CHECK(removed > 10 && pts_removed == (int64_t)box.points.size());   // the box goes, the wall stays

  // a dry run reports it and changes nothing
  prm.dry_run = 1;
  r = a.mapCarve(wall, origin, nullptr, &prm);
  CHECK(a.lastStatus() == NDT_OK);
  CHECK(r.n_rays == (int64_t)wall.points.size() && r.n_rays_skipped == 0 && r.n_steps == steps);
  CHECK(r.n_voxels_crossed == crossed && r.n_voxels_hit == hit && r.n_removed == removed && r.n_points_removed == pts_removed);
  CHECK(a.mapInfo().n_voxels == (int64_t)before.size());

  // the keyframe form on a second engine, the host form (default parameters) on the first: the same survivors
  pclomp::NormalDistributionsTransform<Point, Point> b;
  b.mapReset(leaf);
  b.mapEnableMoments();
  b.mapAdd(wall);
  b.mapAdd(box);
  b.putKeyframe(3, wall);
  const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const ndt_map_carve_result rb = b.mapCarveKeyframe(3, origin, eye);
  CHECK(b.lastStatus() == NDT_OK);
  r = a.mapCarve(wall, origin);
  CHECK(a.lastStatus() == NDT_OK && r.n_removed == removed && r.n_points_removed == pts_removed && r.n_steps == steps);
  CHECK(std::memcmp(&r, &rb, sizeof(r)) == 0);
  ndt_hip::MapState sa, sb;
  a.mapExportState(sa);
  b.mapExportState(sb);
  CHECK(sa.size() == before.size() - (size_t)removed && sa.ijk == sb.ijk && sa.counts == sb.counts);
  size_t w = 0;
  for (size_t i = 0; i < before.size(); ++i) {
    if (!keep[i]) continue;
    CHECK(sa.ijk[3 * w] == before.ijk[3 * i] && sa.ijk[3 * w + 1] == before.ijk[3 * i + 1] && sa.ijk[3 * w + 2] == before.ijk[3 * i + 2]);
    CHECK(sa.counts[w] == before.counts[i]);
    CHECK(std::memcmp(&sa.sums[4 * w], &before.sums[4 * i], 4 * sizeof(float)) == 0);
    CHECK(std::memcmp(&sa.moments[9 * w], &before.moments[9 * i], 9 * sizeof(double)) == 0);
    CHECK(std::memcmp(&sb.sums[4 * w], &before.sums[4 * i], 4 * sizeof(float)) == 0);
    ++w;
  }
  CHECK(w == sa.size() && a.mapInfo().n_points == (int64_t)wall.points.size());

  // refusals: a parameter out of range, a keyframe that is not there, no origin -- each with the map as it was
  ndt_map_carve_default_params(&prm);
  prm.max_steps = 0;
  a.mapCarve(wall, origin, nullptr, &prm);
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG);
  a.mapCarveKeyframe(99, origin, eye);
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG);
  a.mapCarveDevice(nullptr, nullptr, nullptr, 0, nullptr);
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG);
  r = a.mapCarveDevice(nullptr, nullptr, nullptr, 0, origin);      // no rays: a no-op
  CHECK(a.lastStatus() == NDT_OK && r.n_rays == 0 && r.n_removed == 0);
  CHECK(a.mapInfo().n_voxels == (int64_t)sa.size());

  std::printf("map carve: PASS (%zu voxels, %lld removed with %lld points, %lld steps)\n", before.size(), (long long)removed,
              (long long)pts_removed, (long long)steps);
  return 0;
}
