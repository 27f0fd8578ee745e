// The C++ adapter's unprojection surface with PCL- and Eigen-typed arguments (API mocks, tests/cpp/mock), the way a driver
// binds it: beam angles -> scanModelFromBeams -> setScanModel once, then per frame the decoded range image ->
// putKeyframeFromRanges -> setInputSourceFromKeyframe.  Repeats through the adapter
//   the organised form with no trajectory against fmaf on the host, bit for bit, NaN exactly where a pixel is invalid;
//   fused equals composed: unproject with knots and a filter returns the bits of deskew() on the organised cloud;
//   the host form and the keyframe form give the same bits (the keyframe is read back through
//   setInputSourceFromKeyframe + ndt_transform_source with the identity), and replacing the keyframe that is the
//   viewed source unsets the source;
//   refusals: no model, sizes that do not match, times that do not increase.
// Needs a GPU.  Prints "unproject: PASS" and returns 0 when everything agrees.
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

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main() {
  Engine ndt;
  const int n_cols = 61, n_rows = 37;
  const size_t n = (size_t)n_cols * n_rows;
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> u01(0.0f, 1.0f);
  std::vector<uint32_t> range(n);
  std::vector<uint8_t> refl(n);
  std::vector<float> col_t(n_cols);
  for (size_t i = 0; i < n; ++i) {
    range[i] = u01(rng) < 0.2f ? 0u : (uint32_t)(1.0f + 200000.0f * u01(rng));
    refl[i] = (uint8_t)(255.0f * u01(rng));
  }
  for (int c = 0; c < n_cols; ++c) col_t[c] = -0.1f + 1.2f * (float)c / (float)n_cols;   // outside the knots on either side too
  col_t[7] = std::nanf("");                                                              // a column that never arrived
  const std::vector<double> no_times;
  const std::vector<Eigen::Matrix4d> no_poses;

  // ---- no model: refused ----
  CHECK((ndt.unproject<Cloud>(range, refl, col_t, no_times, no_poses).points.empty()) && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  CHECK(ndt.scanModelPixels() == 0);

  // ---- the model from beam angles, the mounting of a driver ----
  std::vector<float> az(n_rows), alt(n_rows);
  for (int r = 0; r < n_rows; ++r) { az[r] = 2.1f - 0.11f * (float)r; alt[r] = 10.7f - 0.6f * (float)r; }
  const Eigen::Matrix4d mount = pose(0.3, -0.1, 0.45, 0.02, -0.01);
  Engine::ScanModel model;
  CHECK(Engine::scanModelFromBeams(n_cols, az, alt, 27.397, &mount, model));
  CHECK(model.n_cols == n_cols && model.n_rows == n_rows && model.x1.size() == n && model.z2.size() == (size_t)n_cols);
  CHECK(!Engine::scanModelFromBeams(0, az, alt, 27.397, nullptr, model) && model.n_cols == n_cols);
  ndt.setScanModel(model);
  CHECK(ndt.lastStatus() == NDT_OK);
  int c_got = 0, r_got = 0;
  CHECK(ndt.scanModelPixels(&c_got, &r_got) == n && c_got == n_cols && r_got == n_rows);

  // ---- the organised form, no trajectory: fmaf on the host, bit for bit ----
  ndt_range_gate gate;
  std::memset(&gate, 0, sizeof(gate));
  gate.use_range = 1; gate.range_min = 1.0f; gate.range_max = 150.0f; gate.row_step = 2;
  std::vector<float> times;
  std::vector<int32_t> index;
  const Cloud organised = ndt.unproject<Cloud>(range, refl, col_t, no_times, no_poses, nullptr, &gate, nullptr, &times, &index);
  CHECK(ndt.lastStatus() == NDT_OK && organised.points.size() == n && times.size() == n && index.size() == n);
  size_t n_valid = 0;
  for (size_t i = 0; i < n; ++i) {
    const int col = (int)(i / n_rows), row = (int)(i % n_rows);
    const float rm = (float)range[i] * 0.001f;
    const bool valid = range[i] != 0 && row % 2 == 0 && std::isfinite(col_t[col]) && 1.0f <= rm && rm <= 150.0f;
    const Point& p = organised.points[i];
    CHECK(index[i] == (int32_t)i && same_bits(times[i], col_t[col]) && p.intensity == (float)refl[i]);
    if (!valid) { CHECK(std::isnan(p.x) && std::isnan(p.y) && std::isnan(p.z)); continue; }
    ++n_valid;
    CHECK(same_bits(p.x, std::fmaf(rm, model.x1[i], model.x2[col])) && same_bits(p.y, std::fmaf(rm, model.y1[i], model.y2[col])) &&
          same_bits(p.z, std::fmaf(rm, model.z1[i], model.z2[col])));
  }
  CHECK(n_valid > n / 8 && n_valid < n / 2);

  // ---- fused equals composed; the host form and the keyframe form agree ----
  std::vector<Eigen::Matrix4d> poses;
  std::vector<double> knots;
  for (int k = 0; k < 22; ++k) {
    const double s = (double)k / 21.0;
    knots.push_back(s);
    poses.push_back(pose(10.0 + 1.0 * s, 2.0 + 0.05 * s * s, 0.3 + 0.01 * s, 0.4 + 0.052 * s, 0.01 * s));
  }
  ndt_scan_filter keep_all;
  std::memset(&keep_all, 0, sizeof(keep_all));
  ndt_scan_filter box = keep_all;
  box.use_box = 1;
  for (int a = 0; a < 3; ++a) { box.box_min[a] = -30.0f; box.box_max[a] = 30.0f; }
  box.use_z_or_intensity = 1;
  box.z_min = -5.0f; box.z_max = 5.0f; box.intensity_keep_min = 200.0f;
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const Eigen::Matrix4d ref = poses[3];
  for (const ndt_scan_filter* f : {(const ndt_scan_filter*)nullptr, (const ndt_scan_filter*)&keep_all, (const ndt_scan_filter*)&box}) {
    std::vector<int32_t> fused_index, composed_index;
    std::vector<float> fused_t;
    const Cloud fused = ndt.unproject<Cloud>(range, refl, col_t, knots, poses, &ref, &gate, f, &fused_t, &fused_index);
    CHECK(ndt.lastStatus() == NDT_OK);
    const Cloud composed = ndt.deskew(organised, times, knots, poses, &ref, f, &composed_index);
    CHECK(ndt.lastStatus() == NDT_OK);
    CHECK(fused.points.size() == composed.points.size() && fused_index == composed_index);
    CHECK(f ? fused.points.size() <= n_valid && !fused.points.empty() : fused.points.size() == n);
    if (f == &keep_all) CHECK(fused.points.size() == n_valid);
    size_t moved = 0, finite = 0;
    for (size_t i = 0; i < fused.points.size(); ++i) {
      const Point &a = fused.points[i], &b = composed.points[i];
      CHECK(std::memcmp(&a.x, &b.x, 12) == 0 && same_bits(a.intensity, b.intensity) && same_bits(fused_t[i], times[fused_index[i]]));
      finite += !std::isnan(a.x);
      moved += !std::isnan(a.x) && a.x != organised.points[fused_index[i]].x;
    }
    CHECK(finite == (f == &box ? fused.points.size() : n_valid) && moved > finite / 2);
    // the keyframe form: a null filter archives what the zeroed filter selects
    const Cloud want = f ? fused : ndt.unproject<Cloud>(range, refl, col_t, knots, poses, &ref, &gate, &keep_all);
    const size_t kept = ndt.putKeyframeFromRanges(9, range, refl, col_t, knots, poses, &ref, &gate, f);
    CHECK(ndt.lastStatus() == NDT_OK && kept == want.points.size());
    ndt.setInputSourceFromKeyframe(9);
    CHECK(ndt.lastStatus() == NDT_OK);
    std::vector<float> back(3 * kept + 3);
    CHECK(ndt_transform_source(ndt.handle(), I, back.data(), kept) == NDT_OK);
    for (size_t i = 0; i < kept; ++i) CHECK(std::memcmp(&want.points[i].x, &back[3 * i], 12) == 0);
    // replacing the keyframe that is the viewed source unsets the source
    CHECK(ndt.putKeyframeFromRanges(9, range, refl, col_t, knots, poses, &ref, &gate, f) == kept);
    CHECK(ndt_source_size(ndt.handle()) == 0);
  }
  // without reflectivities: xyz only, the same points
  const Cloud bare = ndt.unproject<Cloud>(range, std::vector<uint8_t>(), col_t, knots, poses, &ref, &gate, &keep_all);
  const Cloud full = ndt.unproject<Cloud>(range, refl, col_t, knots, poses, &ref, &gate, &keep_all);
  CHECK(bare.points.size() == full.points.size() && !bare.points.empty());
  for (size_t i = 0; i < bare.points.size(); ++i) CHECK(std::memcmp(&bare.points[i].x, &full.points[i].x, 12) == 0 && bare.points[i].intensity == 0.0f);

  // ---- refusals through the adapter; the archive keeps its keyframe ----
  std::vector<float> short_t(col_t.begin(), col_t.begin() + 5);
  CHECK(ndt.unproject<Cloud>(range, refl, short_t, knots, poses).points.empty() && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  std::vector<uint32_t> short_r(range.begin(), range.begin() + 100);
  CHECK(ndt.putKeyframeFromRanges(9, short_r, refl, col_t, knots, poses) == 0 && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  std::vector<double> bad_knots = knots;
  bad_knots[3] = bad_knots[2];
  CHECK(ndt.putKeyframeFromRanges(9, range, refl, col_t, bad_knots, poses) == 0 && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  ndt_range_gate bad_gate = gate;
  bad_gate.row_step = -1;
  CHECK(ndt.unproject<Cloud>(range, refl, col_t, knots, poses, nullptr, &bad_gate).points.empty() && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  CHECK(ndt.keyframeCount() == 1);
  ndt.clearScanModel();
  CHECK(ndt.lastStatus() == NDT_OK && ndt.scanModelPixels() == 0);
  CHECK(ndt.putKeyframeFromRanges(9, range, refl, col_t, knots, poses) == 0 && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  CHECK(ndt.keyframeCount() == 1);
  std::printf("unproject: PASS\n");
  return 0;
}
