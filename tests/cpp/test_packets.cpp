// The C++ adapter's packet surface with PCL- and Eigen-typed arguments (API mocks, tests/cpp/mock), the way a driver binds
// it: setScanModel + setPacketFormat once, then per frame beginPacketFrame, pushPackets as the socket delivers
// (std::vector<uint8_t> payloads, the lidar callback's DataBuffer) and putKeyframeFromPackets.  Through the adapter:
//   unprojectPacketFrame equals unproject() fed a plain host decode of the same payloads, bit for bit, organised and
//   compacting, with each point's time, pixel index, signal and nir;
//   putKeyframeFromPackets archives what putKeyframeFromRanges archives;
//   a packet of the next frame stops pushPackets, and after beginPacketFrame the next frame decodes on its own;
//   refusals: no format, no accepted column, a frame overfull, times that do not increase.
// Needs a GPU.  Prints "packets: PASS" and returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/ndt_omp.h>

#include <Eigen/Core>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                         \
    }                                                                   \
  } while (0)

using Point = pcl::PointXYZI;
using Cloud = pcl::PointCloud<Point>;
using Engine = pclomp::NormalDistributionsTransform<Point, Point>;

namespace {

constexpr int N_COLS = 48, N_ROWS = 21, CPP = 8;
constexpr size_t BLOCK = 12 + 12 * N_ROWS, PACKET = 64 + CPP * BLOCK;

struct Frame {
  std::vector<uint32_t> range;
  std::vector<uint8_t> refl;
  std::vector<uint16_t> signal, nir;
  std::vector<uint64_t> ts;
};

void put(uint8_t* p, uint64_t v, int bytes) {
  for (int b = 0; b < bytes; ++b) p[b] = (uint8_t)(v >> (8 * b));
}

Frame make_frame(unsigned seed, uint64_t t0) {
  std::mt19937 rng(seed);
  Frame f;
  const size_t n = (size_t)N_COLS * N_ROWS;
  f.range.resize(n); f.refl.resize(n); f.signal.resize(n); f.nir.resize(n); f.ts.resize(N_COLS);
  for (size_t i = 0; i < n; ++i) {
    f.range[i] = rng() % 5 == 0 ? 0u : 1u + rng() % 200000u;
    f.refl[i] = (uint8_t)rng();
    f.signal[i] = (uint16_t)rng();
    f.nir[i] = (uint16_t)rng();
  }
  for (int c = 0; c < N_COLS; ++c) f.ts[c] = t0 + 20000000ull * (uint64_t)c;   // 20 ms a column: 0.96 s a frame
  return f;
}

// RNG19 payloads of the frame, random bits wherever the format reads none
std::vector<std::vector<uint8_t>> encode(const Frame& f, int frame_id, unsigned seed) {
  std::mt19937 rng(seed);
  std::vector<std::vector<uint8_t>> out;
  for (int k = 0; k < N_COLS / CPP; ++k) {
    std::vector<uint8_t> p(PACKET);
    for (uint8_t& b : p) b = (uint8_t)rng();
    put(p.data(), 1, 2);
    put(p.data() + 2, (uint64_t)frame_id, 2);
    for (int c = 0; c < CPP; ++c) {
      const int m = k * CPP + c;
      uint8_t* b = p.data() + 32 + (size_t)c * BLOCK;
      put(b, f.ts[m], 8);
      put(b + 8, (uint64_t)m, 2);
      b[10] |= 1;
      for (int r = 0; r < N_ROWS; ++r) {
        const size_t i = (size_t)m * N_ROWS + r;
        uint8_t* px = b + 12 + 12 * (size_t)r;
        put(px, f.range[i] | ((uint64_t)(rng() & 0x1FFFu) << 19), 4);
        px[4] = f.refl[i];
        put(px + 6, f.signal[i], 2);
        put(px + 8, f.nir[i], 2);
      }
    }
    out.push_back(p);
  }
  return out;
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

Eigen::Matrix4d pose(double x, double y, double yaw) {
  Eigen::Matrix4d T = Eigen::Matrix4d::Identity();
  T(0, 0) = std::cos(yaw); T(0, 1) = -std::sin(yaw); T(1, 0) = std::sin(yaw); T(1, 1) = std::cos(yaw);
  T(0, 3) = x; T(1, 3) = y;
  return T;
}

}  // namespace

int main() {
  Engine ndt;
  const size_t n = (size_t)N_COLS * N_ROWS;
  std::vector<float> az(N_ROWS), alt(N_ROWS);
  for (int r = 0; r < N_ROWS; ++r) { az[r] = 2.1f - 0.11f * (float)r; alt[r] = 10.7f - 0.9f * (float)r; }
  Engine::ScanModel model;
  CHECK(Engine::scanModelFromBeams(N_COLS, az, alt, 27.397, nullptr, model));
  const std::vector<double> no_times;
  const std::vector<Eigen::Matrix4d> no_poses;

  // ---- no model, no format: refused ----
  ndt.setPacketFormat(NDT_LIDAR_PROFILE_RNG19, CPP);
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG && ndt.packetSize() == 0);
  ndt.setScanModel(model);
  CHECK(ndt.lastStatus() == NDT_OK);
  ndt.beginPacketFrame();
  CHECK(ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  ndt.setPacketFormat(NDT_LIDAR_PROFILE_RNG19, CPP);
  CHECK(ndt.lastStatus() == NDT_OK && ndt.packetSize() == PACKET);

  // ---- frame 7 and the first packet of frame 8, as the socket delivers them ----
  const Frame fa = make_frame(1, 1700000000ull * 1000000000ull), fb = make_frame(2, 1700000001ull * 1000000000ull);
  std::vector<std::vector<uint8_t>> pa = encode(fa, 7, 3), pb = encode(fb, 8, 4);
  pa[2][32 + 3 * BLOCK + 10] &= 0xFE;                                   // column 19 arrives with an invalid status
  ndt.beginPacketFrame();
  CHECK(ndt.lastStatus() == NDT_OK);
  CHECK((ndt.unprojectPacketFrame<Cloud>(no_times, no_poses).points.empty()) && ndt.lastStatus() == NDT_ERR_INVALID_ARG);   // no accepted column
  std::vector<std::vector<uint8_t>> stream = pa;
  stream.push_back(pb[0]);
  CHECK(ndt.pushPackets(stream) == pa.size() && ndt.lastStatus() == NDT_OK);
  ndt_packet_frame_info info = ndt.packetFrameInfo();
  CHECK(info.frame_id == 7 && info.next_frame_pending == 1 && info.n_columns == N_COLS - 1 && info.n_columns_bad_status == 1);
  CHECK(info.n_packets == (int64_t)pa.size());

  // the plain host decode of frame 7: what the range-image calls take
  std::vector<float> col_t(N_COLS);
  const double t_ref = std::fmod((double)fa.ts[0] * 1e-9, 86400.0);
  for (int c = 0; c < N_COLS; ++c) col_t[c] = (float)std::fmax(0.0, std::fmod((double)fa.ts[c] * 1e-9, 86400.0) - t_ref);
  col_t[19] = std::nanf("");
  std::vector<uint32_t> range = fa.range;
  std::vector<uint8_t> refl = fa.refl;
  std::vector<uint16_t> sig_img = fa.signal, nir_img = fa.nir;
  for (int r = 0; r < N_ROWS; ++r) range[19 * N_ROWS + r] = 0, refl[19 * N_ROWS + r] = 0, sig_img[19 * N_ROWS + r] = 0, nir_img[19 * N_ROWS + r] = 0;
  CHECK(info.t_ref == t_ref);

  std::vector<Eigen::Matrix4d> poses;
  std::vector<double> knots;
  for (int k = 0; k < 22; ++k) {
    const double s = (double)k / 21.0;
    knots.push_back(s);
    poses.push_back(pose(10.0 + 1.0 * s, 2.0 + 0.05 * s * s, 0.4 + 0.052 * s));
  }
  ndt_range_gate gate;
  std::memset(&gate, 0, sizeof(gate));
  gate.use_range = 1; gate.range_min = 1.0f; gate.range_max = 150.0f; gate.row_step = 2;
  ndt_scan_filter keep_all;
  std::memset(&keep_all, 0, sizeof(keep_all));
  ndt_scan_filter box = keep_all;
  box.use_box = 1;
  for (int a = 0; a < 3; ++a) { box.box_min[a] = -30.0f; box.box_max[a] = 30.0f; }
  box.use_z_or_intensity = 1;
  box.z_min = -5.0f; box.z_max = 5.0f; box.intensity_keep_min = 200.0f;
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (const ndt_scan_filter* f : {(const ndt_scan_filter*)nullptr, (const ndt_scan_filter*)&keep_all, (const ndt_scan_filter*)&box}) {
    std::vector<float> t_want, t_got;
    std::vector<int32_t> i_want, i_got;
    std::vector<uint16_t> sig, nir;
    const Cloud want = ndt.unproject<Cloud>(range, refl, col_t, knots, poses, nullptr, &gate, f, &t_want, &i_want);
    CHECK(ndt.lastStatus() == NDT_OK);
    const Cloud got = ndt.unprojectPacketFrame<Cloud>(knots, poses, nullptr, &gate, f, &t_got, &i_got, &sig, &nir);
    CHECK(ndt.lastStatus() == NDT_OK);
    CHECK(got.points.size() == want.points.size() && i_got == i_want && sig.size() == got.points.size() && nir.size() == sig.size());
    CHECK(f ? (!got.points.empty() && got.points.size() < n) : got.points.size() == n);
    for (size_t i = 0; i < got.points.size(); ++i) {
      CHECK(std::memcmp(&got.points[i].x, &want.points[i].x, 12) == 0 && same_bits(got.points[i].intensity, want.points[i].intensity));
      CHECK(same_bits(t_got[i], t_want[i]) && sig[i] == sig_img[i_got[i]] && nir[i] == nir_img[i_got[i]]);
    }
    // the keyframe form
    const size_t kept_r = ndt.putKeyframeFromRanges(9, range, refl, col_t, knots, poses, nullptr, &gate, f);
    CHECK(ndt.lastStatus() == NDT_OK);
    ndt.setInputSourceFromKeyframe(9);
    std::vector<float> back_r(3 * kept_r + 3), back_p(3 * kept_r + 3);
    CHECK(ndt_transform_source(ndt.handle(), I, back_r.data(), kept_r) == NDT_OK);
    std::vector<uint16_t> ksig;
    const size_t kept_p = ndt.putKeyframeFromPackets(10, knots, poses, nullptr, &gate, f, &ksig);
    CHECK(ndt.lastStatus() == NDT_OK && kept_p == kept_r && ksig.size() == kept_p && kept_p > 0);
    ndt.setInputSourceFromKeyframe(10);
    CHECK(ndt_transform_source(ndt.handle(), I, back_p.data(), kept_p) == NDT_OK);
    CHECK(std::memcmp(back_r.data(), back_p.data(), 12 * kept_r) == 0);
    if (f) CHECK(ksig == sig);
  }

  // ---- the next frame: begin, push the packet that stopped the last push and the rest, one by one ----
  ndt.beginPacketFrame();
  CHECK(ndt.lastStatus() == NDT_OK && ndt.packetFrameInfo().frame_id == -1);
  for (const std::vector<uint8_t>& p : pb) CHECK(ndt.pushPackets(p) == 1);
  CHECK(ndt.packetFrameInfo().frame_id == 8 && ndt.packetFrameInfo().n_columns == N_COLS);
  std::vector<int32_t> idx;
  std::vector<uint16_t> sig;
  const Cloud org = ndt.unprojectPacketFrame<Cloud>(no_times, no_poses, nullptr, nullptr, nullptr, nullptr, &idx, &sig);
  CHECK(ndt.lastStatus() == NDT_OK && org.points.size() == n && sig == fb.signal);
  for (size_t i = 0; i < n; ++i) {
    CHECK(org.points[i].intensity == (float)fb.refl[i] && idx[i] == (int32_t)i);
    if (fb.range[i] == 0) { CHECK(std::isnan(org.points[i].x)); continue; }
    const float rm = (float)fb.range[i] * 0.001f;
    CHECK(same_bits(org.points[i].x, std::fmaf(rm, model.x1[i], model.x2[i / N_ROWS])));
  }

  // ---- refusals: a frame overfull, times that do not increase, a new model ----
  CHECK(ndt.pushPackets(pb) == pb.size());                                // the capacity: two frames' worth
  const ndt_packet_frame_info full = ndt.packetFrameInfo();
  CHECK(full.n_packets_accepted == 2 * (int64_t)pb.size() && full.n_columns_overridden == N_COLS);
  CHECK(ndt.pushPackets(pb[0]) == 0 && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  CHECK(ndt.packetFrameInfo().n_packets == full.n_packets);
  std::vector<double> bad_knots = knots;
  bad_knots[3] = bad_knots[2];
  const auto archived = ndt.keyframeCount();
  CHECK(ndt.putKeyframeFromPackets(11, bad_knots, poses) == 0 && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  CHECK((ndt.unprojectPacketFrame<Cloud>(bad_knots, poses).points.empty()) && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  CHECK(ndt.keyframeCount() == archived);
  ndt.setScanModel(model);                                                // drops the format and the frame
  CHECK(ndt.lastStatus() == NDT_OK && ndt.packetSize() == 0);
  CHECK(ndt.pushPackets(pb[0]) == 0 && ndt.lastStatus() == NDT_ERR_INVALID_ARG);
  std::printf("packets: PASS\n");
  return 0;
}
