// The C++ adapter's Scan Context surface (setScanContextParams, scanContext, scanContextKeyframe, scanContextBank*,
// scanContextMatch, scanContextMatchKeyframe, scanContextYaw) with PCL-typed clouds (API mocks, tests/cpp/mock): two places
// are archived as keyframes, their descriptors go into the bank, and a scan of the first place taken under another heading
// finds it again together with that heading -- the way a loop-closure driver would ask.
// Scene: around the sensor a closed wall whose distance and height vary with the azimuth, seeded per place.
// Needs a GPU.  Prints "scan_context: PASS" and returns 0 when everything agrees.
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <pclomp/ndt_omp.h>

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

using Point = pcl::PointXYZ;
using Cloud = pcl::PointCloud<Point>;
using Ndt = pclomp::NormalDistributionsTransform<Point, Point>;

// n points of place `seed` as a sensor yawed by `yaw` sees them: a wall at 8 .. 60 m whose distance and height change every
// 10 degrees of azimuth, and ground returns in front of it
static Cloud place(int n, unsigned seed, double yaw) {
  std::mt19937 shape(seed), rng(seed + 1000);
  double dist[36], hgt[36];
  std::uniform_real_distribution<double> d(8.0, 60.0), h(1.0, 12.0), u(0.0, 1.0);
  for (int k = 0; k < 36; ++k) { dist[k] = d(shape); hgt[k] = h(shape); }
  Cloud out;
  for (int i = 0; i < n; ++i) {
    const double az = 2.0 * M_PI * u(rng);
    const int k = (int)(az / (2.0 * M_PI) * 36.0) % 36;
    const bool ground = i % 3 == 0;
    const double r = ground ? dist[k] * u(rng) : dist[k], z = ground ? -1.8 : -1.8 + hgt[k] * u(rng);
    Point q{};
    q.x = (float)(r * std::cos(az - yaw));   // the world at azimuth az appears at az - yaw
    q.y = (float)(r * std::sin(az - yaw));
    q.z = (float)z;
    out.points.push_back(q);
  }
  return out;
}

int main() {
  const int k_true = 17;                                             // the query's heading in sectors of 6 degrees
  const double yaw_true = k_true * 2.0 * M_PI / 60.0;
  const Cloud a0 = place(20000, 5, 0.0), b0 = place(20000, 9, 0.0), query_cloud = place(20000, 5, yaw_true);

  Ndt n;
  CHECK(n.lastStatus() == NDT_OK);
  ndt_scan_context_params def;
  ndt_scan_context_default_params(&def);
  const ndt_scan_context_params prm = n.getScanContextParams();
  CHECK(n.lastStatus() == NDT_OK && std::memcmp(&prm, &def, sizeof(def)) == 0 && prm.n_rings == 20 && prm.n_sectors == 60);
  const size_t bins = 1200;

  // an empty bank matches nothing
  CHECK(n.scanContextBankCount() == 0);
  CHECK(n.scanContextMatch(std::vector<float>(bins, 1.0f)).size() == 0 && n.lastStatus() == NDT_OK);
  n.scanContextMatchKeyframe(0);
  CHECK(n.lastStatus() == NDT_ERR_INVALID_ARG);

  // two places archived; their descriptors enter the bank under the keyframes' ids
  n.putKeyframe(0, a0);
  n.putKeyframe(1, b0);
  CHECK(n.lastStatus() == NDT_OK);
  std::vector<int32_t> counts;
  const std::vector<float> da = n.scanContextKeyframe(0, &counts);
  CHECK(n.lastStatus() == NDT_OK && da.size() == bins && counts.size() == bins);
  long total = 0;
  float top = 0.0f;
  for (size_t i = 0; i < bins; ++i) { total += counts[i]; CHECK(da[i] >= 0.0f && (counts[i] > 0 || da[i] == 0.0f)); top = std::max(top, da[i]); }
  CHECK(total == 20000 && top > 6.0f && top < 12.3f);                // every point within 80 m; heights -1.8 + up to 12, lifted by 2
  const std::vector<float> db = n.scanContextKeyframe(1);
  CHECK(n.lastStatus() == NDT_OK && db.size() == bins && n.scanContextBankCount() == 2);
  n.scanContextKeyframe(5);
  CHECK(n.lastStatus() == NDT_ERR_INVALID_ARG && n.scanContextBankCount() == 2);

  // the host form gives the keyframe form's bits
  std::vector<int32_t> counts_host;
  const std::vector<float> da_host = n.scanContext(a0, &counts_host);
  CHECK(n.lastStatus() == NDT_OK && da_host.size() == bins && std::memcmp(da_host.data(), da.data(), bins * sizeof(float)) == 0);
  CHECK(counts_host == counts);
  const std::vector<float> none = n.scanContext(Cloud());
  CHECK(n.lastStatus() == NDT_OK && none == std::vector<float>(bins, 0.0f));

  // the place seen under another heading is found, and the heading with it
  const std::vector<float> dq = n.scanContext(query_cloud);
  CHECK(n.lastStatus() == NDT_OK);
  const auto m = n.scanContextMatch(dq);
  CHECK(n.lastStatus() == NDT_OK && m.size() == 2 && m.ids[0] == 0 && m.ids[1] == 1);
  std::printf("scan context: place 0 at %.4f (shift %d, %d columns), place 1 at %.4f (shift %d)\n", m.distance[0], m.shift[0],
              m.columns[0], m.distance[1], m.shift[1]);
  CHECK(m.best() == 0 && m.distance[0] < 0.1 && m.distance[1] > 2.0 * m.distance[0] && m.distance[1] <= 1.0);
  CHECK(m.shift[0] == k_true && m.columns[0] > 50 && m.columns[0] <= 60);
  CHECK(std::fabs(Ndt::scanContextYaw(m.shift[0], prm.n_sectors) - yaw_true) < 1e-12);

  // a bank entry as the query: itself at distance ~0 and shift 0
  const auto self = n.scanContextMatchKeyframe(1);
  CHECK(n.lastStatus() == NDT_OK && self.size() == 2 && self.best() == 1 && std::fabs(self.distance[1]) < 1e-12 && self.shift[1] == 0);
  CHECK(self.distance[0] > 0.05);

  // saved descriptors go back in; ids come back ascending
  const std::vector<float> got = n.scanContextBankGet(1);
  CHECK(n.lastStatus() == NDT_OK && got == db);
  n.scanContextBankPut(7, got);
  n.scanContextBankPut(-3, dq);
  CHECK(n.lastStatus() == NDT_OK && n.scanContextBankCount() == 4);
  const auto four = n.scanContextMatchKeyframe(7);
  CHECK(four.size() == 4 && four.ids[0] == -3 && four.ids[1] == 0 && four.ids[2] == 1 && four.ids[3] == 7);
  CHECK(four.distance[2] == four.distance[3] && four.shift[2] == 0 && four.shift[3] == 0);        // two identical entries
  CHECK(four.distance[2] == self.distance[1]);                                                    // ... as in the bank of two
  n.scanContextBankPut(8, std::vector<float>(bins - 1, 0.0f));
  CHECK(n.lastStatus() == NDT_ERR_INVALID_ARG && n.scanContextBankCount() == 4);
  CHECK(n.scanContextMatch(std::vector<float>(7, 0.0f)).size() == 0 && n.lastStatus() == NDT_ERR_INVALID_ARG);

  // erasing: a bank entry goes, the archive's keyframe does not take its descriptor with it
  n.scanContextBankErase(1);
  CHECK(n.lastStatus() == NDT_OK && n.scanContextBankCount() == 3);
  CHECK(n.scanContextBankGet(1).empty() && n.lastStatus() == NDT_ERR_INVALID_ARG);
  n.scanContextBankErase(1);
  CHECK(n.lastStatus() == NDT_ERR_INVALID_ARG);
  n.eraseKeyframe(0);
  CHECK(n.lastStatus() == NDT_OK && n.scanContextBankCount() == 3 && n.scanContextBankGet(0) == da);

  // parameters: a refused set changes nothing, the same set keeps the bank, a change clears it
  ndt_scan_context_params bad = prm;
  bad.z_sign = 0.5f;
  n.setScanContextParams(bad);
  CHECK(n.lastStatus() == NDT_ERR_INVALID_ARG && n.scanContextBankCount() == 3);
  n.setScanContextParams(prm);
  CHECK(n.lastStatus() == NDT_OK && n.scanContextBankCount() == 3);
  ndt_scan_context_params wide = prm;
  wide.n_sectors = 64;
  wide.n_rings = 8;
  n.setScanContextParams(wide);
  CHECK(n.lastStatus() == NDT_OK && n.scanContextBankCount() == 0 && n.getScanContextParams().n_sectors == 64);
  CHECK(n.scanContext(a0).size() == 8 * 64 && n.lastStatus() == NDT_OK);
  n.scanContextBankClear();
  CHECK(n.lastStatus() == NDT_OK);

  // the yaw of a shift, wrapped to (-pi, pi]
  CHECK(Ndt::scanContextYaw(0, 60) == 0.0 && std::fabs(Ndt::scanContextYaw(30, 60) - M_PI) < 1e-15);
  CHECK(std::fabs(Ndt::scanContextYaw(31, 60) + 29.0 * 2.0 * M_PI / 60.0) < 1e-15 && Ndt::scanContextYaw(59, 60) < 0.0);

  std::printf("scan_context: PASS\n");
  return 0;
}
