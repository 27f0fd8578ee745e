// ndt_packets.cpp -- the host pre-pass over a lidar frame's UDP payloads and ndt_packet_columns (plain C++, host only: no
// handle, no device).  The rules are the lidar callback's (ref: src/lidarcallback.cpp:382-447 LEGACY, :632-701 RNG19):
// size and type of a packet, the frame id that ends a frame, per column the measurement id, the status and the
// timestamp.  Every read is a byte-wise little-endian load inside a packet whose size has been checked against the
// format's; no pixel is touched.
#include "ndt_packets.h"

#include <cmath>
#include <limits>

namespace ndt {
namespace pkt {

namespace {

inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }
inline uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

}  // namespace

bool format_make(int profile, int cpp, int n_cols, int n_rows, Format* f) {
  if (profile != NDT_LIDAR_PROFILE_RNG19 && profile != NDT_LIDAR_PROFILE_LEGACY) return false;
  if (cpp < 1 || n_cols < 1 || n_rows < 1) return false;
  const bool legacy = profile == NDT_LIDAR_PROFILE_LEGACY;
  Format g;
  g.profile = profile; g.cpp = cpp; g.n_cols = n_cols; g.n_rows = n_rows;
  g.header = legacy ? 0 : 32;
  g.first_pixel = legacy ? 16 : 12;
  g.block = g.first_pixel + 12 * (size_t)n_rows + (legacy ? 4 : 0);
  g.packet = (legacy ? 0 : 64) + (size_t)cpp * g.block;
  g.slot = (g.packet + 15) & ~(size_t)15;
  g.capacity = 2 * (((size_t)n_cols + (size_t)cpp - 1) / (size_t)cpp);
  // col_src is an int32 dword offset into capacity * slot bytes
  if (g.capacity * (g.slot / 4) > (size_t)std::numeric_limits<int32_t>::max()) return false;
  *f = g;
  return true;
}

void Pass::begin(const Format& fmt) {
  f = fmt;
  src.assign((size_t)(fmt.n_cols > 0 ? fmt.n_cols : 0), -1);
  ts.assign(src.size(), 0.0);
  ts_ref = 0.0;
  slots = 0;
  info = ndt_packet_frame_info{};
  info.frame_id = -1;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  info.t_ref = info.ts_first = info.ts_last = nan;
}

Taken Pass::take(const uint8_t* p, size_t bytes) {
  const bool legacy = f.profile == NDT_LIDAR_PROFILE_LEGACY;
  if (bytes != f.packet) {
    ++info.n_packets;
    ++info.n_packets_bad_size;
    return REJECTED;
  }
  if (!legacy && le16(p) != 0x0001u) {
    ++info.n_packets;
    ++info.n_packets_bad_type;
    return REJECTED;
  }
  const int32_t frame = (int32_t)le16(p + (legacy ? 10 : 2));   // LEGACY: of the packet's FIRST column
  if (info.frame_id >= 0 && frame != info.frame_id) {
    info.next_frame_pending = 1;
    return NEXT_FRAME;
  }
  info.frame_id = frame;
  ++info.n_packets;
  ++info.n_packets_accepted;
  const size_t slot = slots++;
  for (int c = 0; c < f.cpp; ++c) {
    const uint8_t* b = p + f.header + (size_t)c * f.block;
    const uint32_t m_id = le16(b + 8);
    if (m_id >= (uint32_t)f.n_cols) {
      ++info.n_columns_bad_id;
      continue;
    }
    if (legacy) {
      if ((int32_t)le16(b + 10) != frame) {
        ++info.n_columns_bad_frame;
        continue;
      }
      if (le32(b + 16 + 12 * (size_t)f.n_rows) != 0xFFFFFFFFu) {
        ++info.n_columns_bad_status;
        continue;
      }
    } else if (!(b[10] & 1)) {
      ++info.n_columns_bad_status;
      continue;
    }
    const double t = std::fmod((double)le64(b) * 1e-9, 86400.0);
    if (info.n_columns == 0) {   // the first accepted column in arrival order
      ts_ref = t;
      info.ts_first = t;
    }
    info.ts_last = t;
    if (src[m_id] >= 0)
      ++info.n_columns_overridden;   // the LAST arrival of a measurement id holds
    else
      ++info.n_columns;
    // inside the packed buffer by construction: slot < capacity, and the column's pixels end inside its packet
    src[m_id] = (int32_t)((slot * f.slot + f.header + (size_t)c * f.block + f.first_pixel) / 4);
    ts[m_id] = t;
  }
  return ACCEPTED;
}

void Pass::finish(double t_ref, int32_t* col_src, float* col_t, ndt_packet_frame_info* out) const {
  const bool any = info.n_columns > 0;
  const double ref = std::isfinite(t_ref) ? t_ref : (any ? ts_ref : std::numeric_limits<double>::quiet_NaN());
  for (size_t m = 0; m < src.size(); ++m) {
    if (col_src) col_src[m] = src[m];
    if (col_t) col_t[m] = src[m] >= 0 ? (float)std::fmax(0.0, ts[m] - ref) : std::numeric_limits<float>::quiet_NaN();
  }
  if (out) {
    *out = info;
    out->t_ref = ref;
  }
}

}  // namespace pkt
}  // namespace ndt

extern "C" int ndt_packet_columns(int profile, int columns_per_packet, int n_cols, int n_rows, const uint8_t* packets,
                                  const size_t* bytes_each, size_t n_packets, size_t stride_bytes, double t_ref, int32_t* col_src,
                                  float* col_t, ndt_packet_frame_info* info) {
  using namespace ndt::pkt;
  if (!col_src || !col_t || !info) return NDT_ERR_INVALID_ARG;
  if (n_packets && (!packets || !bytes_each)) return NDT_ERR_INVALID_ARG;
  if (std::isinf(t_ref)) return NDT_ERR_INVALID_ARG;   // (NaN: automatic)
  Format f;
  if (!format_make(profile, columns_per_packet, n_cols, n_rows, &f)) return NDT_ERR_INVALID_ARG;
  for (size_t k = 0; k < n_packets; ++k)
    if (bytes_each[k] > stride_bytes) return NDT_ERR_INVALID_ARG;   // a packet does not fit its place in the array
  Pass pass;
  pass.begin(f);
  for (size_t k = 0; k < n_packets; ++k) {
    if (pass.slots == f.capacity) break;   // the packed buffer is full: the rest is not taken (info->n_packets says so)
    if (pass.take(packets + k * stride_bytes, bytes_each[k]) == NEXT_FRAME) break;
  }
  pass.finish(t_ref, col_src, col_t, info);
  return NDT_OK;
}
