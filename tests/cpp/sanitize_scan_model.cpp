// csrc/ndt_scan_model.cpp (host only) under AddressSanitizer + UBSan as a stand-alone program: the tables are written
// into heap buffers of exactly n_cols * n_rows and n_cols floats, at the shapes of tests/test_unproject_cpu.py, so a
// write past either end is caught; plus the refusals, which must write nothing.  Prints PASS and returns 0.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "ndt_hip.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main() {
  const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const double mount[16] = {0.0, 1.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.3, -0.2, 0.45, 1.0};   // a quarter turn
  const int shapes[3][2] = {{1, 1}, {7, 3}, {2048, 128}};
  for (const auto& s : shapes) {
    const int n_cols = s[0], n_rows = s[1];
    const size_t n = (size_t)n_cols * n_rows;
    std::vector<float> az(n_rows), alt(n_rows);
    for (int r = 0; r < n_rows; ++r) { az[r] = 2.09f - 0.03f * (float)r; alt[r] = 10.74f - 0.17f * (float)r; }
    for (const double* T : {eye, mount}) {
      std::vector<float> x1(n), y1(n), z1(n), x2(n_cols), y2(n_cols), z2(n_cols);
      CHECK(ndt_scan_model_from_beams(n_cols, n_rows, az.data(), alt.data(), 27.397, T, x1.data(), y1.data(), z1.data(), x2.data(),
                                      y2.data(), z2.data()) == NDT_OK);
      for (size_t i = 0; i < n; ++i) {
        const double len = std::sqrt((double)x1[i] * x1[i] + (double)y1[i] * y1[i] + (double)z1[i] * z1[i]);
        CHECK(std::fabs(len - 1.0) < 1e-6);
      }
      // the quarter turn maps the lidar's x onto the body's y (column-major: column 0 of `mount` is (0, 1, 0))
      if (T == mount) {
        std::vector<float> a1(n), b1(n), c1(n), a2(n_cols), b2(n_cols), c2(n_cols);
        CHECK(ndt_scan_model_from_beams(n_cols, n_rows, az.data(), alt.data(), 27.397, eye, a1.data(), b1.data(), c1.data(), a2.data(),
                                        b2.data(), c2.data()) == NDT_OK);
        for (size_t i = 0; i < n; ++i) CHECK(y1[i] == a1[i] && x1[i] == -b1[i] && z1[i] == c1[i]);
      }
    }
  }
  // refusals: nothing written
  std::vector<float> az(3, 1.0f), alt(3, 2.0f), o(21, -1.0f), c(7, -1.0f);
  auto call = [&](int n_cols, int n_rows, const float* a, const float* b, double mm, const double* T, float* x1) {
    return ndt_scan_model_from_beams(n_cols, n_rows, a, b, mm, T, x1, o.data(), o.data(), c.data(), c.data(), c.data());
  };
  CHECK(call(7, 3, nullptr, alt.data(), 27.0, eye, o.data()) == NDT_ERR_INVALID_ARG);
  CHECK(call(7, 3, az.data(), nullptr, 27.0, eye, o.data()) == NDT_ERR_INVALID_ARG);
  CHECK(call(7, 3, az.data(), alt.data(), 27.0, nullptr, o.data()) == NDT_ERR_INVALID_ARG);
  CHECK(call(7, 3, az.data(), alt.data(), 27.0, eye, nullptr) == NDT_ERR_INVALID_ARG);
  CHECK(call(0, 3, az.data(), alt.data(), 27.0, eye, o.data()) == NDT_ERR_INVALID_ARG);
  CHECK(call(7, 0, az.data(), alt.data(), 27.0, eye, o.data()) == NDT_ERR_INVALID_ARG);
  CHECK(call(65536, 32768, az.data(), alt.data(), 27.0, eye, o.data()) == NDT_ERR_INVALID_ARG);
  CHECK(call(7, 3, az.data(), alt.data(), std::numeric_limits<double>::quiet_NaN(), eye, o.data()) == NDT_ERR_INVALID_ARG);
  double bad[16];
  for (int e = 0; e < 16; ++e) bad[e] = eye[e];
  bad[13] = std::numeric_limits<double>::infinity();
  CHECK(call(7, 3, az.data(), alt.data(), 27.0, bad, o.data()) == NDT_ERR_INVALID_ARG);
  az[2] = std::numeric_limits<float>::infinity();
  CHECK(call(7, 3, az.data(), alt.data(), 27.0, eye, o.data()) == NDT_ERR_INVALID_ARG);
  for (float v : o) CHECK(v == -1.0f);
  for (float v : c) CHECK(v == -1.0f);
  std::printf("PASS\n");
  return 0;
}
