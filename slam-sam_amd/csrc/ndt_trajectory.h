// ndt_trajectory.h -- the pose trajectory a scan is deskewed along (internal; plain C++, no HIP in it: the functions
// marked NDT_TRAJ_HD compile for the host with any C++ compiler and, inside a .hip file, for the device as well).
//
// A trajectory is n knots (time, pose body -> map).  Relative to a reference pose `ref` every knot is reduced on the
// host to D_k = ref^-1 T_k as a unit quaternion q_k (sign: q_k . q_{k-1} >= 0) and a translation d_k; per segment
// [k, k+1] the half-angle theta_k = atan2(|vec(conj(q_k) q_{k+1})|, scalar part) and 1 / sin(theta_k).  The pose at time
// t (clamped to the knots' range) is the slerp of the quaternions and the linear blend of the translations at
// u = (t - t_k) / (t_{k+1} - t_k); below NLERP_BELOW the slerp is the normalised linear blend.  A segment whose two knots
// reduce to bit-equal (q, d) is RIGID: its pose is (q_k, d_k) itself, no interpolation arithmetic -- "no motion" is exact.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NDT_TRAJ_HD __host__ __device__
#else
#define NDT_TRAJ_HD
#endif

namespace ndt {
namespace traj {

constexpr int MAX_KNOTS = 64;           // NDT_DESKEW_MAX_KNOTS
constexpr double NLERP_BELOW = 1e-8;    // half-angle below which slerp and the normalised blend agree beyond f64 at 300 m

// One knot, and the segment that starts at it.  12 doubles: the table goes to the device as it is.
struct KnotRow {
  double t;
  double q[4];        // w, x, y, z
  double d[3];
  double theta;       // half-angle of the segment [this knot, next knot]
  double inv_sin;     // 1 / sin(theta); unused where theta < NLERP_BELOW
  int32_t rigid;      // the next knot has the same (q, d) bit for bit (also set on the last knot)
  int32_t identity;   // (q, d) = ((1, 0, 0, 0), 0) exactly
  double pad;
};
static_assert(sizeof(KnotRow) == 12 * sizeof(double), "KnotRow is 12 doubles");
constexpr int ROW_WORDS = 12;

// the segment of a time inside the knots' range: the largest k <= n - 2 with rows[k].t <= t (0 for a single knot)
NDT_TRAJ_HD inline int segment_of(const KnotRow* rows, int n, double t) {
  int lo = 0, hi = n - 2;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].t <= t) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// D(t) as quaternion and translation; returns true where the pose is the exact identity of a rigid segment
NDT_TRAJ_HD inline bool pose_at(const KnotRow* rows, int n, double t, double q[4], double d[3]) {
  const double t0 = rows[0].t, t1 = rows[n - 1].t;
  t = t < t0 ? t0 : (t > t1 ? t1 : t);
  const int k = segment_of(rows, n, t);
  const KnotRow& a = rows[k];
  if (a.rigid) {
    for (int i = 0; i < 4; ++i) q[i] = a.q[i];
    for (int i = 0; i < 3; ++i) d[i] = a.d[i];
    return a.identity != 0;
  }
  const KnotRow& b = rows[k + 1];
  const double u = (t - a.t) / (b.t - a.t);
  if (a.theta < NLERP_BELOW) {
    double s = 0.0;
    for (int i = 0; i < 4; ++i) {
      q[i] = (1.0 - u) * a.q[i] + u * b.q[i];
      s += q[i] * q[i];
    }
    s = 1.0 / sqrt(s);
    for (int i = 0; i < 4; ++i) q[i] *= s;
  } else {
    // (both arguments lie in [0, theta], theta <= pi / 2)
    const double wa = sin((1.0 - u) * a.theta) * a.inv_sin, wb = sin(u * a.theta) * a.inv_sin;
    for (int i = 0; i < 4; ++i) q[i] = wa * a.q[i] + wb * b.q[i];
  }
  for (int i = 0; i < 3; ++i) d[i] = a.d[i] + u * (b.d[i] - a.d[i]);
  return false;
}

// rotation matrix of a unit quaternion, row-major
NDT_TRAJ_HD inline void quat_to_rot(const double q[4], double R[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// The table of a trajectory (ndt_trajectory.cpp).  knot_poses16: n 4 x 4 doubles, column-major; ref16: the pose the
// scan is expressed in, null = the last knot.  A knot whose pose equals the reference bit for bit reduces to the exact
// identity.  Returns 0, or NDT_ERR_INVALID_ARG with *why naming the reason: a null pointer, n outside 1 .. MAX_KNOTS,
// times not strictly increasing, a non-finite time or pose entry.
int build_rows(const double* knot_t, const double* knot_poses16, int n, const double* ref16, KnotRow* rows, const char** why);

}  // namespace traj
}  // namespace ndt
