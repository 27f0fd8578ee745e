// alignMany through the plain face of include/ndt_hip/ndt_hip.hpp.  Built and run by tests/test_gpu_align_batch.py
// (needs an MI355X):
//   test_align_many <target.f32> <source.f32> <guesses.f32> <out.bin>
// Clouds are packed xyz floats, guesses K x 16 column-major floats.  For every guess out.bin receives the result's pose
// (16 floats, column-major), its Hessian (36 doubles, row-major), iteration_num (int32), transform_probability and
// nearest_voxel_transformation_likelihood (2 floats).  Exit code 0 = the call succeeded and the adapter's own
// align() result was left alone.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "ndt_hip/ndt_hip.hpp"

using PointT = ndt_hip::PointXYZ;
using Cloud = ndt_hip::PointCloud<PointT>;

static std::vector<float> read_floats(const char* path) {
  std::vector<float> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  float x;
  while (std::fread(&x, sizeof(x), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}

static std::shared_ptr<Cloud> cloud(const std::vector<float>& xyz) {
  auto c = std::make_shared<Cloud>();
  for (size_t i = 0; i + 2 < xyz.size(); i += 3) c->points.push_back(PointT{xyz[i], xyz[i + 1], xyz[i + 2], 1.0f});
  return c;
}

int main(int argc, char** argv) {
  if (argc != 5) { std::printf("usage: %s target source guesses out\n", argv[0]); return 2; }
  const std::vector<float> t = read_floats(argv[1]), s = read_floats(argv[2]), g = read_floats(argv[3]);
  if (t.empty() || s.empty() || g.empty() || g.size() % 16) { std::printf("FAIL: inputs\n"); return 2; }
  ndt_hip::NormalDistributionsTransform<PointT, PointT> ndt;
  if (ndt.lastStatus() != NDT_OK) { std::printf("FAIL: engine: %s\n", ndt.lastError().c_str()); return 2; }
  ndt.setResolution(1.0f);
  ndt.setNeighborhoodSearchMethod(ndt_hip::DIRECT7);
  ndt.setMaximumIterations(35);
  ndt.setTransformationEpsilon(1e-4);
  ndt.setStepSize(0.1);
  ndt.setInputTarget(cloud(t));
  ndt.setInputSource(cloud(s));
  std::vector<ndt_hip::Matrix4f> guesses(g.size() / 16);
  for (size_t k = 0; k < guesses.size(); ++k)
    for (int i = 0; i < 16; ++i) guesses[k][i] = g[16 * k + (size_t)i];
  Cloud o;
  ndt.align(o, guesses[0]);
  const ndt_hip::Matrix4f before = ndt.getFinalTransformation();
  const int iters_before = ndt.getFinalNumIteration();
  const std::vector<ndt_hip::NdtResult> rs = ndt.alignMany(guesses);
  if (ndt.lastStatus() != NDT_OK || rs.size() != guesses.size()) {
    std::printf("FAIL: alignMany: %d %s\n", ndt.lastStatus(), ndt.lastError().c_str());
    return 1;
  }
  const ndt_hip::Matrix4f after = ndt.getFinalTransformation();
  for (int i = 0; i < 16; ++i)
    if (before[i] != after[i]) { std::printf("FAIL: alignMany changed getFinalTransformation\n"); return 1; }
  if (ndt.getFinalNumIteration() != iters_before) { std::printf("FAIL: alignMany changed the iteration count\n"); return 1; }
  FILE* f = std::fopen(argv[4], "wb");
  if (!f) return 2;
  for (const auto& r : rs) {
    float T[16];
    double H[36];
    ndt_hip::detail::to_colmajor(r.pose, 4, 4, T);
    ndt_hip::detail::to_rowmajor(r.hessian, 6, 6, H);
    const int it = r.iteration_num;
    const float sc[2] = {r.transform_probability, r.nearest_voxel_transformation_likelihood};
    std::fwrite(T, sizeof(T), 1, f);
    std::fwrite(H, sizeof(H), 1, f);
    std::fwrite(&it, sizeof(it), 1, f);
    std::fwrite(sc, sizeof(sc), 1, f);
  }
  std::fclose(f);
  std::printf("PASS: %zu results\n", rs.size());
  return 0;
}
