// ndt_host_cloud.h -- the pure host half of the host-cloud boundary (internal; no HIP): the layout rule of a strided
// host cloud, the gathers that read one, the scatter that writes one, and the finiteness test of a pose.  Every host
// form of the API goes through these; the engine half (upload_column, download_strided) is in ndt_handoff.hip.
//
// A strided host cloud is n points stride_bytes apart.  A point starts with x, y, z (three floats); an optional
// intensity float lies intensity_offset_bytes into the point (< 0: none).  Nothing else of a point is read or written,
// and nothing behind the last used field of the last point is touched: a cloud may end there.
#pragma once

#include <stddef.h>

#include <cmath>

namespace ndt {
namespace engine {

// the layout rule; an xyz-only cloud is layout_valid(stride_bytes, -1)
inline bool layout_valid(size_t stride_bytes, long intensity_offset_bytes) {
  if (stride_bytes < 12 || stride_bytes % 4) return false;
  return intensity_offset_bytes < 0 || (intensity_offset_bytes % 4 == 0 && intensity_offset_bytes >= 12 &&
                                        (size_t)intensity_offset_bytes + 4 <= stride_bytes);
}

// dst[i] = the float byte_offset into point i
inline void gather_column(const void* base, size_t n, size_t stride_bytes, size_t byte_offset, float* dst) {
  const char* b = static_cast<const char*>(base) + byte_offset;
  for (size_t i = 0; i < n; ++i) dst[i] = *reinterpret_cast<const float*>(b + i * stride_bytes);
}

inline void gather_xyz(const void* base, size_t n, size_t stride_bytes, float* x, float* y, float* z) {
  const char* b = static_cast<const char*>(base);
  for (size_t i = 0; i < n; ++i) {
    const float* p = reinterpret_cast<const float*>(b + i * stride_bytes);
    x[i] = p[0]; y[i] = p[1]; z[i] = p[2];
  }
}

// columns [x | y | z | (intensity)], col_stride floats apart at cols -> the first m points of a strided cloud
inline void scatter_cloud(const float* cols, size_t col_stride, size_t m, void* out, size_t stride_bytes,
                          long intensity_offset_bytes) {
  char* ob = static_cast<char*>(out);
  const bool has_i = intensity_offset_bytes >= 0;
  for (size_t i = 0; i < m; ++i) {
    float* p = reinterpret_cast<float*>(ob + i * stride_bytes);
    p[0] = cols[i]; p[1] = cols[col_stride + i]; p[2] = cols[2 * col_stride + i];
    if (has_i) *reinterpret_cast<float*>(ob + i * stride_bytes + intensity_offset_bytes) = cols[3 * col_stride + i];
  }
}

// every word of a pose (6 or 16 of them), of a moment row, ... is finite
template <typename T>
inline bool all_finite(const T* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

}  // namespace engine
}  // namespace ndt
