// The C++ adapter's GICP class under its compat name (pclomp::GeneralizedIterativeClosestPoint from
// <pclomp/gicp_omp.h>) with PCL-typed clouds and Eigen poses (API mocks, tests/cpp/mock), driven through a
// pcl::Registration pointer the way RegisterCallback::registration would hold it.
// The scene comes from the file named on the command line (tests/test_gpu_gicp.py writes it): int64 n_target, n_source;
// 16 doubles guess (column-major); float32 target xyz, source xyz.
// Needs a GPU.  Prints the final pose in hexadecimal floating point for the Python test to compare, "gicp: PASS", and
// returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/gicp_omp.h>
#include <pclomp/gicp_omp_impl.hpp>
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
using Gicp = pclomp::GeneralizedIterativeClosestPoint<Point, Point>;

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
  double guess16[16];
  CHECK(std::fread(sizes, sizeof(int64_t), 2, f) == 2 && sizes[0] > 0 && sizes[1] > 0);
  CHECK(std::fread(guess16, sizeof(double), 16, f) == 16);
  Cloud::Ptr target(new Cloud), source(new Cloud);
  CHECK(read_cloud(f, (size_t)sizes[0], *target) && read_cloud(f, (size_t)sizes[1], *source));
  std::fclose(f);
  Eigen::Matrix4f guess;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) guess(r, c) = (float)guess16[4 * c + r];

  Gicp::Ptr gicp(new Gicp);
  CHECK(gicp->lastStatus() == NDT_OK);
  // the NDT side of the same engine, as the Python test sets it
  gicp->setResolution(1.0f);
  gicp->setStepSize(0.1);
  // the reference's configuration and PCL's names
  gicp->setMaxCorrespondenceDistance(5.0);
  gicp->setTransformationEpsilon(1e-4);
  gicp->setCorrespondenceRandomness(20);
  gicp->setMaximumIterations(64);
  gicp->setMaximumOptimizerIterations(20);
  CHECK(gicp->lastStatus() == NDT_OK && gicp->getCorrespondenceRandomness() == 20 && gicp->getMaxCorrespondenceDistance() == 5.0);
  // a value outside its range is refused and reported
  gicp->setCorrespondenceRandomness(3);
  CHECK(gicp->lastStatus() == NDT_ERR_INVALID_ARG);
  gicp->setCorrespondenceRandomness(20);
  CHECK(gicp->lastStatus() == NDT_OK);

  // no clouds yet: the guess comes back, not converged
  Cloud out;
  gicp->computeTransformation(out, guess);
  CHECK(gicp->lastStatus() != NDT_OK && !gicp->hasConverged() && gicp->getFinalTransformation() == guess);

  // held the way the registration boundary holds its method
  pcl::Registration<Point, Point>::Ptr registration = gicp;
  registration->setInputTarget(target);
  registration->setInputSource(source);
  CHECK(gicp->lastStatus() == NDT_OK);
  registration->align(out, guess);
  CHECK(gicp->lastStatus() == NDT_OK && registration->hasConverged());
  const ndt_gicp_info& info = gicp->gicpInfo();
  CHECK(info.outer_iterations >= 1 && info.inner_iterations >= info.outer_iterations && info.n_pairs > 0);
  CHECK(gicp->getFinalNumIteration() == info.outer_iterations);
  const Eigen::Matrix4f T = registration->getFinalTransformation();
  CHECK(T != guess && std::isfinite(T(0, 3)));
  const double fit = gicp->getFitnessScore();
  CHECK(gicp->lastStatus() == NDT_OK && fit > 0.0 && fit < 1.0);
  float col[16];
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) col[4 * c + r] = T(r, c);
  std::printf("final");
  for (int i = 0; i < 16; ++i) std::printf(" %a", (double)col[i]);
  std::printf("\n");

  // the same call again gives the same bits
  registration->align(out, guess);
  CHECK(registration->getFinalTransformation() == T);

  std::printf("gicp: PASS (%zu points, %d outer, %d inner iterations, %lld pairs)\n", source->points.size(), info.outer_iterations,
              info.inner_iterations, (long long)info.n_pairs);
  return 0;
}
