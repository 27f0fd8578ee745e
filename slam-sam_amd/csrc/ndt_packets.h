// ndt_packets.h -- the host pre-pass over a lidar frame's UDP payloads (plain C++, no device): which packets belong to
// the frame, which of their columns hold, and where each column's first pixel lies in the packed packet buffer.  It reads
// the packet and column HEADERS only (include/ndt_hip.h has the format table, DESIGN 7j the rules); the pixels are
// gathered on the device (ndt_packets.hip).  ndt_packet_columns runs it over an array of packets, the frame calls
// packet by packet -- one implementation (ndt_packets.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/ndt_hip.h"

namespace ndt {
namespace pkt {

// sizes and offsets of one profile at one shape, all multiples of 4
struct Format {
  int profile = -1;                  // -1: none
  int cpp = 0, n_cols = 0, n_rows = 0;
  size_t header = 0;                 // packet header bytes
  size_t block = 0;                  // bytes of one column
  size_t first_pixel = 0;            // from the start of a column to its first pixel
  size_t packet = 0;                 // the payload size that is accepted
  size_t slot = 0;                   // the packet's stride in the packed buffer: `packet` rounded up to 16
  size_t capacity = 0;               // packets a frame may hold: 2 * ceil(n_cols / cpp)
};
// false: a profile, a count or a size out of range (the packed buffer of `capacity` slots must stay below 2^31 dwords:
// col_src is an int32 dword offset)
bool format_make(int profile, int cpp, int n_cols, int n_rows, Format* f);

enum Taken { ACCEPTED, REJECTED, NEXT_FRAME };

// the frame in progress
struct Pass {
  Format f;
  std::vector<int32_t> src;          // n_cols: dword offset of the column's first pixel in the packed buffer, -1: none
  std::vector<double> ts;            // n_cols: the column's time of day in seconds (valid where src >= 0)
  double ts_ref = 0.0;               // ts of the first accepted column in arrival order
  size_t slots = 0;                  // accepted packets = slots of the packed buffer in use
  ndt_packet_frame_info info{};
  void begin(const Format& fmt);
  // one packet in arrival order; ACCEPTED: it goes into slot `slots - 1` of the packed buffer
  Taken take(const uint8_t* p, size_t bytes);
  // col_src and col_t of the frame so far (n_cols each) and the info; t_ref not finite: automatic
  void finish(double t_ref, int32_t* col_src, float* col_t, ndt_packet_frame_info* out) const;
};

}  // namespace pkt
}  // namespace ndt
