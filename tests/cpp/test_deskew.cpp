// The C++ adapter's deskew surface with PCL- and Eigen-typed arguments (API mocks, tests/cpp/mock), the way a driver binds
// it: FrameData -> putKeyframeDeskewed -> setInputSourceFromKeyframe.  Repeats through the adapter
//   anchor 1  every knot equal to the reference: the scan comes back bit for bit (aligned; compacting with a zeroed
//             filter), at sizes around the wave and block boundaries;
//   anchor 4  the host form and the keyframe form give the same bits on the same input (the keyframe is read back
//             through setInputSourceFromKeyframe + ndt_transform_source with the identity), with and without a filter,
//             and replacing the keyframe that is the viewed source unsets the source.
// Needs a GPU.  Prints "deskew: PASS" and returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/ndt_omp.h>

#include <Eigen/Core>

#include <cmath>
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

using Point = pcl::PointXYZI;
using Cloud = pcl::PointCloud<Point>;
using Engine = pclomp::NormalDistributionsTransform<Point, Point>;

static Eigen::Matrix4d pose(double x, double y, double z, double yaw, double pitch) {
  Eigen::Matrix4d Rz = Eigen::Matrix4d::Identity(), Ry = Eigen::Matrix4d::Identity();
  Rz(0, 0) = std::cos(yaw); Rz(0, 1) = -std::sin(yaw); Rz(1, 0) = std::sin(yaw); Rz(1, 1) = std::cos(yaw);
  Ry(0, 0) = std::cos(pitch); Ry(0, 2) = std::sin(pitch); Ry(2, 0) = -std::sin(pitch); Ry(2, 2) = std::cos(pitch);
  Eigen::Matrix4d T = Rz * Ry;
  T(0, 3) = x; T(1, 3) = y; T(2, 3) = z;
  return T;
}

static bool same_xyzi(const Point& a, const Point& b) {
  return std::memcmp(&a.x, &b.x, 12) == 0 && std::memcmp(&a.intensity, &b.intensity, 4) == 0;
}

int main() {
  Engine ndt;
  std::mt19937 rng(5);
  std::uniform_real_distribution<float> u(-120.0f, 120.0f), u01(0.0f, 1.0f);
  auto scan_of = [&](size_t n, std::vector<float>* t) {
    Cloud c;
    t->clear();
    for (size_t i = 0; i < n; ++i) {
      Point p{};
      p.x = u(rng); p.y = u(rng); p.z = 0.1f * u(rng); p.intensity = 255.0f * u01(rng);
      c.points.push_back(p);
      t->push_back(-0.2f + 1.4f * u01(rng));   // outside the knots' range on either side too
    }
    return c;
  };
  ndt_scan_filter keep_all;
  std::memset(&keep_all, 0, sizeof(keep_all));

  // ---- anchor 1: no motion is exact ----
  const Eigen::Matrix4d here = pose(12.5, -3.25, 0.75, 0.7, 0.02);
  std::vector<float> t;
  for (size_t n : {1u, 63u, 64u, 65u, 255u, 256u, 257u, 1025u}) {
    const Cloud scan = scan_of(n, &t);
    for (size_t knots : {1u, 2u, 22u}) {
      std::vector<Eigen::Matrix4d> poses(knots, here);
      std::vector<double> times;
      for (size_t k = 0; k < knots; ++k) times.push_back((double)k / (double)(knots > 1 ? knots - 1 : 1));
      for (const ndt_scan_filter* f : {(const ndt_scan_filter*)nullptr, (const ndt_scan_filter*)&keep_all}) {
        std::vector<int32_t> index;
        const Cloud out = ndt.deskew(scan, t, times, poses, &here, f, &index);
        CHECK(ndt.lastStatus() == NDT_OK);
        CHECK(out.points.size() == n && index.size() == n);
        for (size_t i = 0; i < n; ++i) CHECK(same_xyzi(out.points[i], scan.points[i]) && index[i] == (int32_t)i);
        const Cloud last = ndt.deskew(scan, t, times, poses, nullptr, f);   // reference = last knot
        CHECK(ndt.lastStatus() == NDT_OK && last.points.size() == n);
        for (size_t i = 0; i < n; ++i) CHECK(same_xyzi(last.points[i], scan.points[i]));
      }
    }
  }

  // ---- anchor 4: the host form and the keyframe form agree, bit for bit ----
  const size_t n = 3001;
  Cloud scan = scan_of(n, &t);
  scan.points[17].y = std::nanf("");
  t[40] = std::nanf("");
  std::vector<Eigen::Matrix4d> poses;
  std::vector<double> times;
  for (int k = 0; k < 22; ++k) {
    const double s = (double)k / 21.0;
    times.push_back(s);
    poses.push_back(pose(10.0 + 1.0 * s, 2.0 + 0.05 * s * s, 0.3 + 0.01 * s, 0.4 + 0.052 * s, 0.01 * s));
  }
  Eigen::Matrix4d D;
  CHECK(Engine::trajectoryPose(times, poses, 1.0, D) && (D - Eigen::Matrix4d::Identity()).norm() < 1e-12);
  ndt_scan_filter box = keep_all;
  box.use_box = 1;
  for (int a = 0; a < 3; ++a) { box.box_min[a] = -30.0f; box.box_max[a] = 30.0f; }
  box.use_z_or_intensity = 1;
  box.z_min = -5.0f; box.z_max = 5.0f; box.intensity_keep_min = 200.0f;
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (const ndt_scan_filter* f : {(const ndt_scan_filter*)nullptr, (const ndt_scan_filter*)&keep_all, (const ndt_scan_filter*)&box}) {
    const Cloud host = ndt.deskew(scan, t, times, poses, nullptr, f);
    CHECK(ndt.lastStatus() == NDT_OK);
    CHECK(f ? host.points.size() < n : host.points.size() == n);
    const size_t kept = ndt.putKeyframeDeskewed(7, scan, t, times, poses, nullptr, f);
    CHECK(ndt.lastStatus() == NDT_OK && kept == host.points.size());
    ndt.setInputSourceFromKeyframe(7);
    CHECK(ndt.lastStatus() == NDT_OK);
    std::vector<float> back(3 * kept + 3);
    CHECK(ndt_transform_source(ndt.handle(), I, back.data(), kept) == NDT_OK);
    size_t moved = 0;
    for (size_t i = 0; i < kept; ++i) {
      // (the identity transform of a NaN point is a NaN point: compare bits only where the host form is finite)
      if (std::isnan(host.points[i].x)) { CHECK(std::isnan(back[3 * i])); continue; }
      CHECK(std::memcmp(&host.points[i].x, &back[3 * i], 12) == 0);
      moved += host.points[i].x != scan.points[i].x;
    }
    CHECK(moved > kept / 2);
    // replacing the keyframe that is the viewed source unsets the source
    CHECK(ndt.putKeyframeDeskewed(7, scan, t, times, poses, nullptr, f) == kept);
    CHECK(ndt_source_size(ndt.handle()) == 0);
  }
  // refusals through the adapter: sizes that do not match, times that do not increase; the archive keeps its keyframe
  std::vector<float> short_t(t.begin(), t.begin() + 5);
  CHECK(ndt.deskew(scan, short_t, times, poses).points.empty() && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  std::vector<double> bad_times = times;
  bad_times[3] = bad_times[2];
  CHECK(ndt.putKeyframeDeskewed(7, scan, t, bad_times, poses) == 0 && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  CHECK(ndt.keyframeCount() == 1);
  std::printf("deskew: PASS\n");
  return 0;
}
