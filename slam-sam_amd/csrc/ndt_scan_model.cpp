// ndt_scan_model.cpp -- the unprojection tables of a spinning lidar from its beam angles (ndt_scan_model_from_beams;
// plain C++, host only: no handle, no device).  The arithmetic is the lidar callback's Initialize()
// (ref: src/lidarcallback.cpp:255-327): angles, their sines and cosines and the products of those in float, the
// lidar -> body transform applied in double, one rounding to float.  Built with -ffp-contract=off like the rest of the
// library: every product rounds as written.
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/ndt_hip.h"

extern "C" int ndt_scan_model_from_beams(int n_cols, int n_rows, const float* beam_azimuth_deg, const float* beam_altitude_deg,
                                         double lidar_origin_to_beam_origin_mm, const double lidar_to_body16_colmajor[16],
                                         float* x1, float* y1, float* z1, float* x2, float* y2, float* z2) {
  if (!beam_azimuth_deg || !beam_altitude_deg || !lidar_to_body16_colmajor || !x1 || !y1 || !z1 || !x2 || !y2 || !z2)
    return NDT_ERR_INVALID_ARG;
  if (n_cols < 1 || n_rows < 1 || (int64_t)n_cols * n_rows > (int64_t)std::numeric_limits<int32_t>::max()) return NDT_ERR_INVALID_ARG;
  if (!std::isfinite(lidar_origin_to_beam_origin_mm)) return NDT_ERR_INVALID_ARG;
  for (int e = 0; e < 16; ++e)
    if (!std::isfinite(lidar_to_body16_colmajor[e])) return NDT_ERR_INVALID_ARG;
  for (int r = 0; r < n_rows; ++r)
    if (!std::isfinite(beam_azimuth_deg[r]) || !std::isfinite(beam_altitude_deg[r])) return NDT_ERR_INVALID_ARG;
  const double* T = lidar_to_body16_colmajor;   // T(r, c) = T[4 * c + r]
  const float pi = static_cast<float>(M_PI);
  const float r0 = static_cast<float>(lidar_origin_to_beam_origin_mm) * 0.001f;
  std::vector<float> az(n_rows), cos_alt(n_rows), sin_alt(n_rows);
  for (int r = 0; r < n_rows; ++r) {
    az[r] = beam_azimuth_deg[r] * pi / 180.0f;
    const float alt = beam_altitude_deg[r] * pi / 180.0f;
    cos_alt[r] = std::cos(alt);
    sin_alt[r] = std::sin(alt);
  }
  for (int m = 0; m < n_cols; ++m) {
    const float az_m = 2.0f * pi * (1.0f - (static_cast<float>(m) / static_cast<float>(n_cols)));
    const double ox = (double)(r0 * std::cos(az_m)), oy = (double)(r0 * std::sin(az_m));
    x2[m] = static_cast<float>(T[0] * ox + T[4] * oy + T[12]);
    y2[m] = static_cast<float>(T[1] * ox + T[5] * oy + T[13]);
    z2[m] = static_cast<float>(T[2] * ox + T[6] * oy + T[14]);
    for (int r = 0; r < n_rows; ++r) {
      const float total = az_m + az[r];
      const float c = std::cos(total), s = std::sin(total);
      const double dx = (double)(cos_alt[r] * c), dy = (double)(cos_alt[r] * s), dz = (double)sin_alt[r];
      const size_t i = (size_t)m * (size_t)n_rows + (size_t)r;
      x1[i] = static_cast<float>(T[0] * dx + T[4] * dy + T[8] * dz);
      y1[i] = static_cast<float>(T[1] * dx + T[5] * dy + T[9] * dz);
      z1[i] = static_cast<float>(T[2] * dx + T[6] * dy + T[10] * dz);
    }
  }
  return NDT_OK;
}
