// The C++ adapter's voxelised GICP class (ndt_hip::VoxelizedGeneralizedIterativeClosestPoint from <ndt_hip/ndt_hip.hpp>; the
// reference names no such class, so there is no compat name) with PCL-typed clouds and Eigen poses (API mocks,
// tests/cpp/mock), driven through a pcl::Registration pointer the way RegisterCallback::registration would hold it.
// The scene comes from the file named on the command line (tests/test_gpu_vgicp.py writes it): int64 n_target, n_source;
// 16 doubles guess (column-major); float32 target xyz, source xyz.
// Needs a GPU.  Prints the final pose in hexadecimal floating point for the Python test to compare, "vgicp: PASS", and
// returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <ndt_hip/ndt_hip.hpp>

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
using Vgicp = ndt_hip::VoxelizedGeneralizedIterativeClosestPoint<Point, Point>;

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

  Vgicp::Ptr vgicp(new Vgicp);
  CHECK(vgicp->lastStatus() == NDT_OK);
  // the NDT loop of the same engine, as the Python test sets it: here PCL's two names are the NDT class's
  vgicp->setResolution(1.0f);
  vgicp->setStepSize(0.1);
  vgicp->setTransformationEpsilon(1e-4);
  vgicp->setMaximumIterations(35);
  vgicp->setNeighborhoodSearchMethod(ndt_hip::DIRECT1);
  CHECK(vgicp->lastStatus() == NDT_OK && vgicp->params().max_iterations == 35 && vgicp->params().trans_epsilon == 1e-4);
  // the covariances are GICP's
  vgicp->setCorrespondenceRandomness(20);
  CHECK(vgicp->lastStatus() == NDT_OK && vgicp->getCorrespondenceRandomness() == 20);
  CHECK(vgicp->gicpParams().max_iterations == 64);   // (the outer loop of GICP: not touched, not read)

  // no clouds yet: the guess comes back, not converged
  Cloud out;
  vgicp->computeTransformation(out, guess);
  CHECK(vgicp->lastStatus() != NDT_OK && !vgicp->hasConverged() && vgicp->getFinalTransformation() == guess);

  // held the way the registration boundary holds its method
  pcl::Registration<Point, Point>::Ptr registration = vgicp;
  registration->setInputTarget(target);
  registration->setInputSource(source);
  CHECK(vgicp->lastStatus() == NDT_OK);
  registration->align(out, guess);
  CHECK(vgicp->lastStatus() == NDT_OK && registration->hasConverged());
  const ndt_vgicp_info& info = vgicp->vgicpInfo();
  CHECK(info.n_voxels > 0 && info.n_voxels <= info.n_leaves && info.n_target_points_in_voxels >= info.n_voxels);
  CHECK(info.n_pairs > 0 && info.n_source_with_pairs > 0 && info.n_source_with_pairs <= info.n_pairs);
  CHECK(info.n_source_with_pairs <= (int64_t)source->points.size());
  CHECK(vgicp->gicpInfo().outer_iterations == 0);   // GICP's align never ran
  const Eigen::Matrix4f T = registration->getFinalTransformation();
  CHECK(T != guess && std::isfinite(T(0, 3)));
  const double fit = vgicp->getFitnessScore();
  CHECK(vgicp->lastStatus() == NDT_OK && fit > 0.0 && fit < 1.0);
  float col[16];
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) col[4 * c + r] = T(r, c);
  std::printf("final");
  for (int i = 0; i < 16; ++i) std::printf(" %a", (double)col[i]);
  std::printf("\n");

  // the same call again gives the same bits
  registration->align(out, guess);
  CHECK(registration->getFinalTransformation() == T);

  std::printf("vgicp: PASS (%zu points, %d iterations, %lld voxels, %lld pairs of %lld points)\n", source->points.size(),
              vgicp->getFinalNumIteration(), (long long)info.n_voxels, (long long)info.n_pairs, (long long)info.n_source_with_pairs);
  return 0;
}
