// The C++ adapter's continuous-time surface (setInputSourceTimes, computeDerivativesCT, alignContinuousTime,
// getDeskewedSource) with PCL-typed clouds and Eigen poses (API mocks, tests/cpp/mock): a scan captured in motion is
// registered with its begin pose known, the way a lidar-only driver would chain its scans.
// The scene comes from the file named on the command line (tests/test_gpu_ct.py writes it): int64 n_target, n_source; 6
// doubles begin pose; 16 doubles guess (column-major); float32 target xyz, source xyz, source times.
// Needs a GPU.  Prints the end pose and the sum of the deskewed scan in hexadecimal floating point for the Python test
// to compare, "ct: PASS", and returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/ndt_omp.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
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

static bool read_cloud(std::FILE* f, size_t n, Cloud& out) {
  std::vector<float> xyz(3 * n);
  if (std::fread(xyz.data(), sizeof(float), 3 * n, f) != 3 * n) return false;
  for (size_t i = 0; i < n; ++i) {
    Point q{};
    q.x = xyz[3 * i]; q.y = xyz[3 * i + 1]; q.z = xyz[3 * i + 2];
    out.points.push_back(q);
  }
  return true;
}

int main(int argc, char** argv) {
  CHECK(argc == 2);
  std::FILE* f = std::fopen(argv[1], "rb");
  CHECK(f != nullptr);
  int64_t sizes[2];
  double begin6[6], guess16[16];
  CHECK(std::fread(sizes, sizeof(int64_t), 2, f) == 2 && sizes[0] > 0 && sizes[1] > 0);
  CHECK(std::fread(begin6, sizeof(double), 6, f) == 6 && std::fread(guess16, sizeof(double), 16, f) == 16);
  Cloud::Ptr target(new Cloud), source(new Cloud);
  CHECK(read_cloud(f, (size_t)sizes[0], *target) && read_cloud(f, (size_t)sizes[1], *source));
  std::vector<float> alpha((size_t)sizes[1]);
  CHECK(std::fread(alpha.data(), sizeof(float), alpha.size(), f) == alpha.size());
  std::fclose(f);
  Ndt::Pose6 begin;
  for (int i = 0; i < 6; ++i) begin[i] = begin6[i];
  Eigen::Matrix4f guess;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) guess(r, c) = (float)guess16[4 * c + r];

  Ndt n;
  CHECK(n.lastStatus() == NDT_OK);
  n.setResolution(1.0f);
  n.setMaximumIterations(35);
  n.setTransformationEpsilon(1e-4);
  n.setStepSize(0.1);
  n.setInputTarget(target);
  n.setInputSource(source);
  CHECK(n.lastStatus() == NDT_OK && n.sourceTimesCount() == 0);

  // no times yet: the guess comes back, not converged
  Ndt::ContinuousTimeResult none = n.alignContinuousTime(begin, guess);
  CHECK(n.lastStatus() == NDT_ERR_NO_SOURCE && !none.converged && none.pose == guess);
  // a ragged times vector is refused
  n.setInputSourceTimes(std::vector<float>(alpha.begin(), alpha.end() - 1));
  CHECK(n.lastStatus() == NDT_ERR_INVALID_ARG && n.sourceTimesCount() == 0);
  n.setInputSourceTimes(alpha);
  CHECK(n.lastStatus() == NDT_OK && n.sourceTimesCount() == sizes[1]);

  // the objective at the guess: a positive score, a symmetric Hessian; without the Hessian the same score and gradient;
  // the begin pose as a 4 x 4 of the same rotation gives the score of the 6-vector to rounding
  Vector6d p, g, g0;
  Matrix6d H, H0;
  const Ndt::Pose6 gp = Ndt::poseOfMatrix(guess);
  for (int i = 0; i < 6; ++i) p[i] = gp[i];
  const double score = n.computeDerivativesCT(g, H, begin, p);
  CHECK(n.lastStatus() == NDT_OK && score > 0 && g.norm() > 0);
  for (int r = 0; r < 6; ++r)
    for (int q = 0; q < 6; ++q) CHECK(H(r, q) == H(q, r));
  CHECK(H(0, 0) < 0 && H(2, 2) < 0);
  CHECK(n.computeDerivativesCT(g0, H0, begin, p, false) == score && g0 == g && H0 == Matrix6d::Zero());
  Eigen::Matrix4f begin4 = Eigen::Matrix4f::Identity();
  {
    const double sr = std::sin(begin[3]), cr = std::cos(begin[3]), sp = std::sin(begin[4]), cp = std::cos(begin[4]);
    const double sy = std::sin(begin[5]), cy = std::cos(begin[5]);
    const double R[9] = {cp * cy, -cp * sy, sp, cr * sy + sr * sp * cy, cr * cy - sr * sp * sy, -sr * cp,
                         sr * sy - cr * sp * cy, sr * cy + cr * sp * sy, cr * cp};
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) begin4(r, c) = (float)R[3 * r + c];
      begin4(r, 3) = (float)begin[r];
    }
  }
  const double score4 = n.computeDerivativesCT(g0, H0, begin4, p);
  CHECK(n.lastStatus() == NDT_OK && std::fabs(score4 - score) < 1e-3 * std::fabs(score));

  // the align, and the same align with the begin pose handed over as a matrix
  const Ndt::ContinuousTimeResult res = n.alignContinuousTime(begin, guess);
  CHECK(n.lastStatus() == NDT_OK && res.converged && res.iteration_num >= 1);
  const Ndt::ContinuousTimeResult res4 = n.alignContinuousTime(begin4, guess);
  CHECK(n.lastStatus() == NDT_OK && res4.converged);
  double d = 0.0;
  for (int i = 0; i < 3; ++i) d += (res4.end_pose[i] - res.end_pose[i]) * (res4.end_pose[i] - res.end_pose[i]);
  CHECK(std::sqrt(d) < 1e-3);                                                   // (an f32 begin pose: 1e-6 of 20 m)
  Vector6d at, g1;
  Matrix6d H1;
  for (int i = 0; i < 6; ++i) at[i] = res.end_pose[i];
  CHECK(n.computeDerivativesCT(g1, H1, begin, at) > score);                     // (a better pose than the guess)
  std::printf("end_pose %a %a %a %a %a %a\n", res.end_pose[0], res.end_pose[1], res.end_pose[2], res.end_pose[3], res.end_pose[4],
              res.end_pose[5]);

  // the deskewed scan under the result: one point per source point, finite, and with begin == end the scan itself
  Cloud deskewed, same;
  n.getDeskewedSource(begin, res.end_pose, deskewed);
  CHECK(n.lastStatus() == NDT_OK && deskewed.points.size() == source->points.size());
  double sum = 0.0;
  for (const Point& q : deskewed.points) {
    CHECK(std::isfinite(q.x) && std::isfinite(q.y) && std::isfinite(q.z));
    sum += (double)q.x;
    sum += (double)q.y;
    sum += (double)q.z;
  }
  std::printf("deskewed_sum %a\n", sum);
  n.getDeskewedSource(res.end_pose, res.end_pose, same);
  CHECK(n.lastStatus() == NDT_OK && same.points.size() == source->points.size());
  for (size_t i = 0; i < same.points.size(); ++i)
    CHECK(same.points[i].x == source->points[i].x && same.points[i].y == source->points[i].y && same.points[i].z == source->points[i].z);
  n.getDeskewedSource(begin, res.end_pose, same, 2);
  CHECK(n.lastStatus() == NDT_ERR_INVALID_ARG && same.points.empty());

  // a new source drops the times
  n.setInputSource(source);
  CHECK(n.lastStatus() == NDT_OK && n.sourceTimesCount() == 0);
  n.getDeskewedSource(begin, res.end_pose, same);
  CHECK(n.lastStatus() == NDT_ERR_NO_SOURCE && same.points.empty());

  std::printf("ct: PASS (%zu points, %d iterations)\n", source->points.size(), res.iteration_num);
  return 0;
}
