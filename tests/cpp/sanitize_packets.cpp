// The host pre-pass over lidar packets (csrc/ndt_packets.cpp: ndt_packet_columns) as a stand-alone program for
// AddressSanitizer + UBSan (tests/test_packets_cpu.py builds and runs it; never loaded into Python).  Packets are built
// here from the format table of include/ndt_hip.h and live in heap buffers that end with the last packet's last byte; the
// outputs hold exactly n_cols entries.  Both profiles; in order, reversed, one packet dropped, one duplicated, invalid
// status, m_id == n_cols, wrong type, wrong size, a column of another frame id (LEGACY), a packet of the next frame,
// bytes_each of 0, stride < bytes_each, n_rows and cpp at 1, t_ref given and automatic, a frame past its capacity.
// Prints "sanitize_packets: PASS" and returns 0 when the counters are what the packets were built to give.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "ndt_hip.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                         \
    }                                                                   \
  } while (0)

namespace {

struct Shape {
  int profile, n_cols, n_rows, cpp;
  size_t header() const { return profile == NDT_LIDAR_PROFILE_LEGACY ? 0 : 32; }
  size_t first() const { return profile == NDT_LIDAR_PROFILE_LEGACY ? 16 : 12; }
  size_t block() const { return first() + 12 * (size_t)n_rows + (profile == NDT_LIDAR_PROFILE_LEGACY ? 4 : 0); }
  size_t size() const { return (profile == NDT_LIDAR_PROFILE_LEGACY ? 0 : 64) + (size_t)cpp * block(); }
  int packets() const { return (n_cols + cpp - 1) / cpp; }
};

void put(uint8_t* p, uint64_t v, int bytes) {
  for (int b = 0; b < bytes; ++b) p[b] = (uint8_t)(v >> (8 * b));
}

// packet k of the frame: columns k * cpp ..., every byte the format does not define set to 0xA5
std::vector<uint8_t> packet(const Shape& s, int k, int frame_id, int type = 1, int bad_status_col = -1, int bad_id_col = -1,
                            int other_frame_col = -1) {
  std::vector<uint8_t> p(s.size(), 0xA5);
  const bool legacy = s.profile == NDT_LIDAR_PROFILE_LEGACY;
  if (!legacy) {
    put(p.data(), (uint64_t)type, 2);
    put(p.data() + 2, (uint64_t)frame_id, 2);
  }
  for (int c = 0; c < s.cpp; ++c) {
    const int m = k * s.cpp + c;
    uint8_t* b = p.data() + s.header() + (size_t)c * s.block();
    const bool live = m < s.n_cols;
    put(b, 1700000000ull * 1000000000ull + 48828ull * (uint64_t)m, 8);
    put(b + 8, (uint64_t)((live && m != bad_id_col) ? m : s.n_cols), 2);
    const bool ok = live && m != bad_status_col;
    if (legacy) {
      put(b + 10, (uint64_t)(m == other_frame_col ? frame_id + 1 : frame_id), 2);
      put(b + 16 + 12 * (size_t)s.n_rows, ok ? 0xFFFFFFFFull : 0x7FFFFFFFull, 4);
    } else {
      b[10] = ok ? 0xA5 : 0xA4;
    }
  }
  return p;
}

// the packets back to back in a heap buffer of exactly their bytes (stride = the longest), then the pass
struct Run {
  std::vector<int32_t> src;
  std::vector<float> t;
  ndt_packet_frame_info info;
  int rc;
};
Run run(const Shape& s, const std::vector<std::vector<uint8_t>>& packets, double t_ref, size_t stride_override = 0) {
  size_t stride = 1;
  for (const auto& p : packets) stride = p.size() > stride ? p.size() : stride;
  if (stride_override) stride = stride_override;
  const size_t total = packets.empty() ? 0 : (packets.size() - 1) * stride + packets.back().size();
  std::unique_ptr<uint8_t[]> buf(new uint8_t[total ? total : 1]);
  std::unique_ptr<size_t[]> sizes(new size_t[packets.size() ? packets.size() : 1]);
  if (!stride_override) {
    std::memset(buf.get(), 0x5A, total ? total : 1);
    for (size_t k = 0; k < packets.size(); ++k) {
      if (!packets[k].empty()) std::memcpy(buf.get() + k * stride, packets[k].data(), packets[k].size());
      sizes[k] = packets[k].size();
    }
  } else {
    for (size_t k = 0; k < packets.size(); ++k) sizes[k] = packets[k].size();   // (refused before anything is read)
  }
  Run r;
  // exactly n_cols entries each, on the heap
  std::unique_ptr<int32_t[]> src(new int32_t[s.n_cols]);
  std::unique_ptr<float[]> t(new float[s.n_cols]);
  r.rc = ndt_packet_columns(s.profile, s.cpp, s.n_cols, s.n_rows, buf.get(), sizes.get(), packets.size(), stride, t_ref, src.get(),
                            t.get(), &r.info);
  if (r.rc == NDT_OK) {
    r.src.assign(src.get(), src.get() + s.n_cols);
    r.t.assign(t.get(), t.get() + s.n_cols);
  }
  return r;
}

int count_live(const Run& r) {
  int n = 0;
  for (int32_t v : r.src) n += v >= 0;
  return n;
}

int check_shape(const Shape& s) {
  const int K = s.packets();
  const bool legacy = s.profile == NDT_LIDAR_PROFILE_LEGACY;
  const double nan = std::nan("");
  std::vector<std::vector<uint8_t>> in_order;
  for (int k = 0; k < K; ++k) in_order.push_back(packet(s, k, 7));
  const size_t slot_words = ((s.size() + 15) / 16 * 16) / 4;
  // in order, t_ref automatic and given
  Run r = run(s, in_order, nan);
  CHECK(r.rc == NDT_OK && count_live(r) == s.n_cols && r.info.n_columns == s.n_cols && r.info.n_packets == K && r.info.frame_id == 7);
  CHECK(r.info.n_columns_bad_id == (int64_t)K * s.cpp - s.n_cols && r.t[0] == 0.0f && r.info.next_frame_pending == 0);
  for (int m = 0; m < s.n_cols; ++m) {
    CHECK((size_t)r.src[m] == (size_t)(m / s.cpp) * slot_words + (s.header() + (size_t)(m % s.cpp) * s.block() + s.first()) / 4);
    CHECK((size_t)r.src[m] + 3 * (size_t)s.n_rows <= (size_t)K * slot_words);
  }
  Run g = run(s, in_order, r.info.t_ref - 1.5);
  CHECK(g.rc == NDT_OK && g.t[0] == 1.5f && g.info.t_ref == r.info.t_ref - 1.5);
  // reversed: every column before the first arrival clamps to 0
  std::vector<std::vector<uint8_t>> rev(in_order.rbegin(), in_order.rend());
  r = run(s, rev, nan);
  CHECK(r.rc == NDT_OK && count_live(r) == s.n_cols && r.t[0] == 0.0f && r.src[0] >= (int32_t)((K - 1) * slot_words));
  // one dropped, one duplicated (the later arrival holds), invalid status, m_id == n_cols
  if (K > 1) {
    std::vector<std::vector<uint8_t>> dropped(in_order.begin() + 1, in_order.end());
    r = run(s, dropped, nan);
    CHECK(r.rc == NDT_OK && r.src[0] == -1 && std::isnan(r.t[0]) && r.info.n_columns == s.n_cols - s.cpp);
  }
  std::vector<std::vector<uint8_t>> dup = in_order;
  dup.push_back(in_order[0]);
  r = run(s, dup, nan);
  CHECK(r.rc == NDT_OK && r.info.n_columns_overridden == (s.cpp < s.n_cols ? s.cpp : s.n_cols) && r.src[0] >= (int32_t)(K * slot_words));
  std::vector<std::vector<uint8_t>> bad = in_order;
  bad[0] = packet(s, 0, 7, 1, 0, -1);
  r = run(s, bad, nan);
  CHECK(r.rc == NDT_OK && r.info.n_columns_bad_status == 1 && r.src[0] == -1 && r.info.n_columns == s.n_cols - 1);
  bad[0] = packet(s, 0, 7, 1, -1, 0);
  r = run(s, bad, nan);
  CHECK(r.rc == NDT_OK && r.info.n_columns_bad_id == 1 + (int64_t)K * s.cpp - s.n_cols && r.src[0] == -1);
  if (legacy && s.cpp > 1) {
    bad[0] = packet(s, 0, 7, 1, -1, -1, 1);
    r = run(s, bad, nan);
    CHECK(r.rc == NDT_OK && r.info.n_columns_bad_frame == 1 && r.src[1] == -1 && r.src[0] >= 0);
  }
  if (!legacy) {
    bad[0] = packet(s, 0, 7, 2);
    r = run(s, bad, nan);
    CHECK(r.rc == NDT_OK && r.info.n_packets_bad_type == 1 && r.src[0] == -1 && r.info.n_packets == K);
  }
  // wrong sizes: one byte short, one long, empty; the buffer ends with the short packet's last byte
  std::vector<std::vector<uint8_t>> sizes = in_order;
  sizes.push_back(std::vector<uint8_t>(in_order[0].begin(), in_order[0].end() - 1));
  sizes.insert(sizes.begin(), std::vector<uint8_t>());
  sizes.insert(sizes.begin(), std::vector<uint8_t>(s.size() + 1, 0x01));
  sizes.push_back(std::vector<uint8_t>(in_order[0].begin(), in_order[0].begin() + 1));
  r = run(s, sizes, nan);
  CHECK(r.rc == NDT_OK && r.info.n_packets_bad_size == 4 && r.info.n_columns == s.n_cols && r.info.n_packets == K + 4);
  // bytes_each of 0 alone, and no packet at all
  r = run(s, {std::vector<uint8_t>()}, nan);
  CHECK(r.rc == NDT_OK && r.info.n_packets_bad_size == 1 && count_live(r) == 0 && std::isnan(r.info.t_ref) && r.info.frame_id == -1);
  r = run(s, {}, nan);
  CHECK(r.rc == NDT_OK && r.info.n_packets == 0 && count_live(r) == 0);
  // a packet of the next frame stops the pass
  std::vector<std::vector<uint8_t>> two = {in_order[0], packet(s, 0, 8), in_order[K - 1]};
  r = run(s, two, nan);
  CHECK(r.rc == NDT_OK && r.info.next_frame_pending == 1 && r.info.n_packets == 1 && r.info.frame_id == 7);
  // past the capacity: 2 * K packets are taken, the rest is not
  std::vector<std::vector<uint8_t>> many;
  for (int rep = 0; rep < 3; ++rep) many.insert(many.end(), in_order.begin(), in_order.end());
  r = run(s, many, nan);
  CHECK(r.rc == NDT_OK && r.info.n_packets_accepted == 2 * K && r.info.n_packets == 2 * K);
  for (int m = 0; m < s.n_cols; ++m) CHECK((size_t)r.src[m] + 3 * (size_t)s.n_rows <= (size_t)(2 * K) * slot_words);
  // stride < bytes_each: refused, nothing read
  r = run(s, in_order, nan, s.size() - 1);
  CHECK(r.rc == NDT_ERR_INVALID_ARG);
  return 0;
}

}  // namespace

int main() {
  const Shape shapes[] = {{0, 2, 3, 2}, {0, 24, 5, 4}, {0, 10, 4, 4}, {0, 7, 1, 1}, {0, 5, 1, 3}, {0, 3, 2, 1}, {0, 32, 128, 16},
                          {1, 2, 3, 2}, {1, 24, 5, 4}, {1, 10, 4, 4}, {1, 7, 1, 1}, {1, 5, 1, 3}, {1, 3, 2, 1}, {1, 32, 128, 16}};
  for (const Shape& s : shapes)
    if (check_shape(s)) {
      std::printf("at profile %d, %d x %d, cpp %d\n", s.profile, s.n_cols, s.n_rows, s.cpp);
      return 1;
    }
  // refusals: nothing is written
  int32_t src[2] = {-9, -9};
  float t[2] = {-9.0f, -9.0f};
  ndt_packet_frame_info info;
  std::memset(&info, 0x11, sizeof(info));
  uint8_t one[4] = {0, 0, 0, 0};
  size_t four = 4;
  CHECK(ndt_packet_columns(2, 1, 2, 1, one, &four, 1, 4, 0.0, src, t, &info) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 0, 2, 1, one, &four, 1, 4, 0.0, src, t, &info) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 1, 0, 1, one, &four, 1, 4, 0.0, src, t, &info) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 1, 2, 0, one, &four, 1, 4, 0.0, src, t, &info) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 1, 2, 1, nullptr, &four, 1, 4, 0.0, src, t, &info) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 1, 2, 1, one, nullptr, 1, 4, 0.0, src, t, &info) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 1, 2, 1, one, &four, 1, 3, 0.0, src, t, &info) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 1, 2, 1, one, &four, 1, 4, INFINITY, src, t, &info) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 1, 2, 1, one, &four, 1, 4, 0.0, nullptr, t, &info) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 1, 2, 1, one, &four, 1, 4, 0.0, src, nullptr, &info) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 1, 2, 1, one, &four, 1, 4, 0.0, src, t, nullptr) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_packet_columns(0, 1, 65536, 8192, one, &four, 1, 4, 0.0, src, t, &info) == NDT_ERR_INVALID_ARG);
  CHECK(src[0] == -9 && src[1] == -9 && t[0] == -9.0f && t[1] == -9.0f && info.n_packets == 0x1111111111111111ll);
  std::printf("sanitize_packets: PASS\n");
  return 0;
}
