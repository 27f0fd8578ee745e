// sanitize_trajectory.cpp -- the host side of the deskew model (csrc/ndt_trajectory.cpp) under AddressSanitizer + UBSan:
// a stand-alone program, built and run by tests/test_deskew_cpu.py.  It walks ndt_trajectory_pose over trajectories of
// 1, 2, 3 and 64 knots whose segments turn by 1e-10 rad .. 170 deg, at every knot, mid-segment and outside the ends,
// compares with the geodesic R_k Exp(u Log(R_k^T R_{k+1})) from ndt_se3.h, checks the rigid rule and every refusal.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "ndt_hip.h"
#include "ndt_se3.h"
#include "ndt_trajectory.h"

using namespace ndt;

static int failures = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static se3::Pose turn(std::mt19937_64& rng, double angle, double trans) {
  std::normal_distribution<double> g(0.0, 1.0);
  std::uniform_real_distribution<double> u(-trans, trans);
  double ax[3] = {g(rng), g(rng), g(rng)};
  const double n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  // (rotation and translation separately: expmap's translation is V v, not v -- irrelevant here, any pose will do)
  double xi[6] = {angle * ax[0] / n, angle * ax[1] / n, angle * ax[2] / n, 0.0, 0.0, 0.0};
  se3::Pose p = se3::expmap(xi);
  for (int i = 0; i < 3; ++i) p.t[i] = u(rng);
  return p;
}

static void trajectory(int n, uint64_t seed, int shift, std::vector<double>* t, std::vector<double>* poses) {
  static const double rot[5] = {1e-10, 1e-5, 3.0 * M_PI / 180.0, 0.5 * M_PI, 170.0 * M_PI / 180.0};
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> step(0.05, 0.15);
  se3::Pose T = turn(rng, 2.0, 50.0);
  double now = 0.0;
  t->assign(1, now);
  poses->resize(16 * (size_t)n);
  se3::to_colmajor(T, poses->data());
  for (int k = 1; k < n; ++k) {
    T = se3::compose(T, turn(rng, rot[(k - 1 + shift) % 5], 1.0));
    now += step(rng);
    t->push_back(now);
    se3::to_colmajor(T, poses->data() + 16 * (size_t)k);
  }
}

static void check_against_geodesic(const std::vector<double>& t, const std::vector<double>& poses, const double* ref16, double at) {
  const int n = (int)t.size();
  double out[16];
  CHECK(ndt_trajectory_pose(t.data(), poses.data(), n, ref16, at, out) == NDT_OK);
  const se3::Pose ref = se3::from_colmajor(ref16 ? ref16 : poses.data() + 16 * (size_t)(n - 1));
  const double tc = std::fmin(std::fmax(at, t.front()), t.back());
  int k = 0;
  while (k + 2 < n && t[(size_t)k + 1] <= tc) ++k;
  se3::Pose want = se3::between(ref, se3::from_colmajor(poses.data() + 16 * (size_t)k));
  if (n > 1) {
    const se3::Pose b = se3::between(ref, se3::from_colmajor(poses.data() + 16 * (size_t)(k + 1)));
    const double u = (tc - t[(size_t)k]) / (t[(size_t)k + 1] - t[(size_t)k]);
    const se3::Pose rel = se3::between(want, b);
    double xi[6] = {0, 0, 0, 0, 0, 0};
    se3::so3_log(rel.R, xi);
    for (int i = 0; i < 3; ++i) xi[i] *= u;
    const se3::Pose step = se3::expmap(xi);   // (pure rotation)
    se3::Pose r = want;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) r.R[i][j] = want.R[i][0] * step.R[0][j] + want.R[i][1] * step.R[1][j] + want.R[i][2] * step.R[2][j];
      r.t[i] = want.t[i] + u * (b.t[i] - want.t[i]);
    }
    want = r;
  }
  double w16[16];
  se3::to_colmajor(want, w16);
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) CHECK(std::fabs(out[4 * c + r] - w16[4 * c + r]) <= 1e-12);
  for (int r = 0; r < 3; ++r) CHECK(std::fabs(out[12 + r] - w16[12 + r]) <= 1e-12 * (1.0 + std::fabs(w16[12 + r])));
  CHECK(out[3] == 0.0 && out[7] == 0.0 && out[11] == 0.0 && out[15] == 1.0);
}

int main() {
  const int counts[4] = {1, 2, 3, 64};
  std::vector<double> t, poses;
  for (int n : counts)
    for (int shift = 0; shift < 5; ++shift) {
      trajectory(n, 1000u * (unsigned)n + (unsigned)shift, shift, &t, &poses);
      std::vector<double> other(16);
      std::mt19937_64 rng(77u + (unsigned)shift);
      se3::to_colmajor(turn(rng, 1.0, 20.0), other.data());
      const double* refs[3] = {nullptr, poses.data(), other.data()};
      for (const double* ref : refs) {
        for (int k = 0; k < n; ++k) {
          check_against_geodesic(t, poses, ref, t[(size_t)k]);
          if (k + 1 < n) check_against_geodesic(t, poses, ref, 0.5 * (t[(size_t)k] + t[(size_t)k + 1]));
        }
        check_against_geodesic(t, poses, ref, t.front() - 3.0);
        check_against_geodesic(t, poses, ref, t.back() + 3.0);
      }
    }

  // rigid rule: bit-equal neighbouring knots; all knots equal to the reference
  trajectory(4, 5, 2, &t, &poses);
  std::memcpy(poses.data() + 32, poses.data() + 16, 16 * sizeof(double));
  double a[16], b[16];
  CHECK(ndt_trajectory_pose(t.data(), poses.data(), 4, nullptr, t[1], a) == NDT_OK);
  for (double u : {0.0, 0.1, 0.5, 0.9, 1.0}) {
    CHECK(ndt_trajectory_pose(t.data(), poses.data(), 4, nullptr, t[1] + u * (t[2] - t[1]), b) == NDT_OK);
    CHECK(std::memcmp(a, b, sizeof(a)) == 0);
  }
  for (int n : counts) {
    trajectory(1, 9, 0, &t, &poses);
    std::vector<double> same, times;
    for (int k = 0; k < n; ++k) {
      same.insert(same.end(), poses.begin(), poses.end());
      times.push_back((double)k);
    }
    double eye[16];
    se3::to_colmajor(se3::identity(), eye);
    for (double at : {-1.0, 0.0, 0.5, (double)n - 1.0, (double)n + 5.0}) {
      CHECK(ndt_trajectory_pose(times.data(), same.data(), n, nullptr, at, b) == NDT_OK);
      CHECK(std::memcmp(b, eye, sizeof(eye)) == 0);
      CHECK(ndt_trajectory_pose(times.data(), same.data(), n, poses.data(), at, b) == NDT_OK);
      CHECK(std::memcmp(b, eye, sizeof(eye)) == 0);
    }
  }

  // refusals
  trajectory(65, 3, 0, &t, &poses);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  CHECK(ndt_trajectory_pose(t.data(), poses.data(), 64, nullptr, 0.1, a) == NDT_OK);
  CHECK(ndt_trajectory_pose(t.data(), poses.data(), 65, nullptr, 0.1, a) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_trajectory_pose(t.data(), poses.data(), 0, nullptr, 0.1, a) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_trajectory_pose(nullptr, poses.data(), 3, nullptr, 0.1, a) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_trajectory_pose(t.data(), nullptr, 3, nullptr, 0.1, a) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_trajectory_pose(t.data(), poses.data(), 3, nullptr, 0.1, nullptr) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_trajectory_pose(t.data(), poses.data(), 3, nullptr, nan, a) == NDT_ERR_INVALID_ARG);
  CHECK(ndt_trajectory_pose(t.data(), poses.data(), 3, nullptr, inf, a) == NDT_ERR_INVALID_ARG);
  for (double bad : {nan, inf, -inf}) {
    std::vector<double> t2(t.begin(), t.begin() + 3), p2(poses.begin(), poses.begin() + 48);
    t2[1] = bad;
    CHECK(ndt_trajectory_pose(t2.data(), poses.data(), 3, nullptr, 0.1, a) == NDT_ERR_INVALID_ARG);
    p2[16 + 13] = bad;
    CHECK(ndt_trajectory_pose(t.data(), p2.data(), 3, nullptr, 0.1, a) == NDT_ERR_INVALID_ARG);
    CHECK(ndt_trajectory_pose(t.data(), poses.data(), 3, p2.data() + 16, 0.1, a) == NDT_ERR_INVALID_ARG);
  }
  {
    std::vector<double> t2 = {0.0, 0.2, 0.2}, t3 = {0.0, 0.3, 0.2};
    CHECK(ndt_trajectory_pose(t2.data(), poses.data(), 3, nullptr, 0.1, a) == NDT_ERR_INVALID_ARG);
    CHECK(ndt_trajectory_pose(t3.data(), poses.data(), 3, nullptr, 0.1, a) == NDT_ERR_INVALID_ARG);
  }
  // the table builder with every out-parameter, as the engine calls it
  traj::KnotRow rows[traj::MAX_KNOTS];
  const char* why = nullptr;
  CHECK(traj::build_rows(t.data(), poses.data(), 64, nullptr, rows, &why) == NDT_OK);
  CHECK(traj::build_rows(t.data(), poses.data(), 65, nullptr, rows, &why) == NDT_ERR_INVALID_ARG && why != nullptr);
  std::printf(failures ? "%d checks failed\n" : "PASS\n", failures);
  return failures ? 1 : 0;
}
