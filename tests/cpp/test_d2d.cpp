// The C++ adapter's distribution-to-distribution surface (setInputSourceDistributions, getSourceDistributions,
// computeDerivativesD2D, alignDistributions) with PCL-typed clouds and Eigen poses (API mocks, tests/cpp/mock): a submap's
// saved state is registered to the map's target and merged under the pose found, the way a pose-graph driver would.
// Scene: wavy ground and two walls on 30 m x 30 m, leaf 1.0; the submap is another sample of the surfaces in a frame that
// is off by 0.25 m and 1.5 degrees.
// Needs a GPU.  Prints "d2d: PASS" and returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/ndt_omp.h>

#include <cmath>
#include <cstdio>
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
using Vector6d = Eigen::Matrix<double, 6, 1>;
using Matrix6d = Eigen::Matrix<double, 6, 6>;

// n points of the surfaces in the map frame, then moved by `to_frame` (row-major 3 x 4)
static Cloud sample(int n, unsigned seed, const double to_frame[12]) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> u(-15.0, 15.0), h(0.0, 4.0), noise(-0.02, 0.02);
  Cloud out;
  for (int i = 0; i < n; ++i) {
    double p[3];
    const int kind = i % 4;
    if (kind < 2) { p[0] = u(rng); p[1] = u(rng); p[2] = 0.4 * std::sin(p[0] / 3.0) * std::cos(p[1] / 4.0); }
    else if (kind == 2) { p[0] = 6.4; p[1] = u(rng); p[2] = h(rng); }
    else { p[0] = u(rng); p[1] = -7.3; p[2] = h(rng); }
    for (int a = 0; a < 3; ++a) p[a] += noise(rng);
    Point q{};
    q.x = (float)(to_frame[0] * p[0] + to_frame[1] * p[1] + to_frame[2] * p[2] + to_frame[3]);
    q.y = (float)(to_frame[4] * p[0] + to_frame[5] * p[1] + to_frame[6] * p[2] + to_frame[7]);
    q.z = (float)(to_frame[8] * p[0] + to_frame[9] * p[1] + to_frame[10] * p[2] + to_frame[11]);
    out.points.push_back(q);
  }
  return out;
}

static void fresh_map(Ndt& n, const Cloud& cloud) {
  n.setResolution(1.0f);
  n.setMaximumIterations(35);
  n.setTransformationEpsilon(1e-4);
  n.setStepSize(0.1);
  n.mapReset(1.0f);
  n.mapEnableMoments();
  n.mapAdd(cloud);
}

int main() {
  // the submap's frame -> the map's frame: yaw 1.5 degrees, (0.2, -0.12, 0.06); the submap is sampled through the inverse
  const double yaw = 1.5 * M_PI / 180.0, c = std::cos(yaw), s = std::sin(yaw), t[3] = {0.2, -0.12, 0.06};
  const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const double inv[12] = {c, s, 0, -(c * t[0] + s * t[1]), -s, c, 0, -(-s * t[0] + c * t[1]), 0, 0, 1, -t[2]};
  const Cloud map_cloud = sample(24000, 3, ident), sub_cloud = sample(20000, 4, inv);

  Ndt a, b;
  CHECK(a.lastStatus() == NDT_OK && b.lastStatus() == NDT_OK);
  fresh_map(a, map_cloud);
  a.setInputTargetFromMapMoments();
  CHECK(a.lastStatus() == NDT_OK);
  fresh_map(b, sub_cloud);
  ndt_hip::MapState sub;
  b.mapExportState(sub);
  CHECK(b.lastStatus() == NDT_OK && sub.size() > 500 && sub.moments.size() == 9 * sub.size());

  // no distribution source yet: the guess comes back, not converged
  bool converged = true;
  Eigen::Matrix4f guess = Eigen::Matrix4f::Identity();
  guess(0, 3) = 0.01f;
  ndt_hip::NdtResult none = a.alignDistributions(guess, &converged);
  CHECK(a.lastStatus() == NDT_ERR_NO_SOURCE && !converged && none.pose == guess);
  CHECK(a.getSourceDistributions().size() == 0);

  // the submap's records become the source Gaussians: those with at least 6 points and a sound covariance, in input order
  a.setInputSourceDistributions(sub);
  CHECK(a.lastStatus() == NDT_OK);
  const auto src = a.getSourceDistributions();
  CHECK(a.lastStatus() == NDT_OK && src.n_records == (int64_t)sub.size() && src.size() > 300 && src.size() < sub.size());
  CHECK(src.mean.size() == 3 * src.size() && src.cov.size() == 6 * src.size());
  for (size_t i = 0; i < src.size(); ++i) {
    const size_t r = (size_t)src.record_index[i];
    CHECK(r < sub.size() && (i == 0 || src.record_index[i] > src.record_index[i - 1]));
    CHECK(src.counts[i] == sub.counts[r] && src.counts[i] >= 6);
    CHECK(src.mean[3 * i] == sub.moments[9 * r] / (double)sub.counts[r]);      // the leaf's mean: sum / count
    CHECK(src.cov[6 * i] > 0 && src.cov[6 * i + 3] > 0 && src.cov[6 * i + 5] > 0);
  }
  // ragged vectors are refused and the source stays
  std::vector<double> ragged(sub.moments.begin(), sub.moments.end() - 1);
  a.setInputSourceDistributions(sub.counts, ragged);
  CHECK(a.lastStatus() == NDT_ERR_INVALID_ARG && a.getSourceDistributions().size() == src.size());

  // the objective at the identity: a positive score, an uphill gradient, a symmetric Hessian; without the Hessian the same
  // score and gradient
  Vector6d p, g, g0;
  Matrix6d H, H0;
  const double score = a.computeDerivativesD2D(g, H, p);
  CHECK(a.lastStatus() == NDT_OK && score > 0 && g.norm() > 0);
  for (int r = 0; r < 6; ++r)
    for (int q = 0; q < 6; ++q) CHECK(H(r, q) == H(q, r));
  CHECK(H(0, 0) < 0 && H(2, 2) < 0);
  CHECK(a.computeDerivativesD2D(g0, H0, p, false) == score && g0 == g && H0 == Matrix6d::Zero());

  // the align finds the frame offset ...
  const ndt_hip::NdtResult res = a.alignDistributions(Eigen::Matrix4f::Identity(), &converged);
  CHECK(a.lastStatus() == NDT_OK && converged && res.iteration_num >= 1);
  const double dx = res.pose(0, 3) - t[0], dy = res.pose(1, 3) - t[1], dz = res.pose(2, 3) - t[2];
  const double dyaw = std::atan2((double)res.pose(1, 0), (double)res.pose(0, 0)) - yaw;
  std::printf("d2d align: %d iterations, off by %.4f m, %.5f rad in yaw\n", res.iteration_num, std::sqrt(dx * dx + dy * dy + dz * dz), dyaw);
  CHECK(std::sqrt(dx * dx + dy * dy + dz * dz) < 0.05 && std::fabs(dyaw) < 0.005);
  Vector6d g1;
  Matrix6d H1;
  Vector6d at;
  at[0] = res.pose(0, 3); at[1] = res.pose(1, 3); at[2] = res.pose(2, 3);
  at[5] = std::atan2((double)res.pose(1, 0), (double)res.pose(0, 0));
  CHECK(a.computeDerivativesD2D(g1, H1, at) > score);                          // (a better pose than the identity)

  // ... and it is the pose the posed import takes: the submap joins the map
  const int64_t points_before = a.mapInfo().n_points, voxels_before = a.mapInfo().n_voxels;
  a.mapImportStatePosed(sub, res.pose.cast<double>());
  CHECK(a.lastStatus() == NDT_OK && a.mapInfo().n_points == points_before + (int64_t)sub_cloud.points.size());
  CHECK(a.mapInfo().n_voxels >= voxels_before);

  // clearing the source
  a.setInputSourceDistributions(std::vector<int32_t>(), std::vector<double>());
  CHECK(a.lastStatus() == NDT_OK && a.getSourceDistributions().size() == 0);

  std::printf("d2d: PASS (%zu records, %zu Gaussians)\n", sub.size(), src.size());
  return 0;
}
