// ndt_trajectory.cpp -- host side of the deskew model (see ndt_trajectory.h): knot poses -> the table the kernels
// read, and ndt_trajectory_pose.  No device, no handle.
#include "ndt_trajectory.h"

#include <cmath>
#include <cstring>

#include "../../include/ndt_hip.h"
#include "ndt_se3.h"

namespace ndt {
namespace traj {

namespace {

// unit quaternion (w, x, y, z) of a rotation matrix: the branch with the largest pivot, then normalised
void rot_to_quat(const double R[3][3], double q[4]) {
  const double tr = R[0][0] + R[1][1] + R[2][2];
  if (tr > 0.0) {
    const double s = 2.0 * std::sqrt(tr + 1.0);
    q[0] = 0.25 * s;
    q[1] = (R[2][1] - R[1][2]) / s;
    q[2] = (R[0][2] - R[2][0]) / s;
    q[3] = (R[1][0] - R[0][1]) / s;
  } else {
    int m = 0;
    if (R[1][1] > R[m][m]) m = 1;
    if (R[2][2] > R[m][m]) m = 2;
    const int a = (m + 1) % 3, b = (m + 2) % 3;
    const double s = 2.0 * std::sqrt(1.0 + R[m][m] - R[a][a] - R[b][b]);
    q[0] = (R[b][a] - R[a][b]) / s;
    q[1 + m] = 0.25 * s;
    q[1 + a] = (R[a][m] + R[m][a]) / s;
    q[1 + b] = (R[b][m] + R[m][b]) / s;
  }
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) q[i] /= n;
  if (q[0] < 0.0)
    for (int i = 0; i < 4; ++i) q[i] = -q[i];
}

}  // namespace

int build_rows(const double* knot_t, const double* knot_poses16, int n, const double* ref16, KnotRow* rows, const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  if (!knot_t || !knot_poses16 || !rows) { *why = "trajectory: null pointer"; return NDT_ERR_INVALID_ARG; }
  if (n < 1 || n > MAX_KNOTS) { *why = "trajectory: n_knots outside 1 .. NDT_DESKEW_MAX_KNOTS"; return NDT_ERR_INVALID_ARG; }
  for (int k = 0; k < n; ++k) {
    if (!std::isfinite(knot_t[k])) { *why = "trajectory: non-finite knot time"; return NDT_ERR_INVALID_ARG; }
    if (k && !(knot_t[k] > knot_t[k - 1])) { *why = "trajectory: knot times not strictly increasing"; return NDT_ERR_INVALID_ARG; }
    for (int e = 0; e < 16; ++e)
      if (!std::isfinite(knot_poses16[16 * k + e])) { *why = "trajectory: non-finite pose entry"; return NDT_ERR_INVALID_ARG; }
  }
  if (!ref16) ref16 = knot_poses16 + 16 * (size_t)(n - 1);
  for (int e = 0; e < 16; ++e)
    if (!std::isfinite(ref16[e])) { *why = "trajectory: non-finite reference pose entry"; return NDT_ERR_INVALID_ARG; }
  const se3::Pose ref = se3::from_colmajor(ref16);
  for (int k = 0; k < n; ++k) {
    KnotRow& r = rows[k];
    std::memset(&r, 0, sizeof(r));
    r.t = knot_t[k];
    const double* Tk = knot_poses16 + 16 * (size_t)k;
    if (std::memcmp(Tk, ref16, 16 * sizeof(double)) == 0) {   // this knot IS the reference: the identity, exactly
      r.q[0] = 1.0;
      r.identity = 1;
    } else {
      const se3::Pose D = se3::between(ref, se3::from_colmajor(Tk));
      rot_to_quat(D.R, r.q);
      for (int i = 0; i < 3; ++i) r.d[i] = D.t[i];
      r.identity = r.q[0] == 1.0 && r.q[1] == 0.0 && r.q[2] == 0.0 && r.q[3] == 0.0 && r.d[0] == 0.0 && r.d[1] == 0.0 &&
                   r.d[2] == 0.0;
      if (r.identity)   // (no -0.0 in a pose that is compared bit for bit)
        for (int i = 0; i < 3; ++i) r.q[1 + i] = r.d[i] = 0.0;
    }
    if (k) {   // the shorter arc
      const double* p = rows[k - 1].q;
      if (r.q[0] * p[0] + r.q[1] * p[1] + r.q[2] * p[2] + r.q[3] * p[3] < 0.0)
        for (int i = 0; i < 4; ++i) r.q[i] = -r.q[i];
    }
  }
  for (int k = 0; k < n; ++k) {
    KnotRow& a = rows[k];
    if (k == n - 1) { a.rigid = 1; a.theta = 0.0; a.inv_sin = 0.0; break; }
    const KnotRow& b = rows[k + 1];
    a.rigid = std::memcmp(a.q, b.q, sizeof(a.q)) == 0 && std::memcmp(a.d, b.d, sizeof(a.d)) == 0;
    // r = conj(q_a) q_b: the half-angle from atan2, which keeps the small angles acos of the dot product loses
    const double* p = a.q;
    const double* q = b.q;
    const double rw = p[0] * q[0] + p[1] * q[1] + p[2] * q[2] + p[3] * q[3];
    const double rx = p[0] * q[1] - p[1] * q[0] - p[2] * q[3] + p[3] * q[2];
    const double ry = p[0] * q[2] + p[1] * q[3] - p[2] * q[0] - p[3] * q[1];
    const double rz = p[0] * q[3] - p[1] * q[2] + p[2] * q[1] - p[3] * q[0];
    a.theta = std::atan2(std::sqrt(rx * rx + ry * ry + rz * rz), rw);
    a.inv_sin = a.theta < NLERP_BELOW ? 0.0 : 1.0 / std::sin(a.theta);
  }
  // (a sign flip for the shorter arc leaves an identity row (-1, 0, 0, 0): the same pose, no longer the exact pattern)
  for (int k = 0; k < n; ++k)
    if (rows[k].identity && rows[k].q[0] != 1.0) rows[k].identity = 0;
  return NDT_OK;
}

}  // namespace traj
}  // namespace ndt

extern "C" int ndt_trajectory_pose(const double* knot_t, const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
                                   double t, double out_pose16[16]) {
  using namespace ndt::traj;
  if (!out_pose16 || !std::isfinite(t)) return NDT_ERR_INVALID_ARG;
  KnotRow rows[MAX_KNOTS];
  const int rc = build_rows(knot_t, knot_poses16, n_knots, ref_pose16_or_null, rows, nullptr);
  if (rc) return rc;
  double q[4], d[3], R[9];
  pose_at(rows, n_knots, t, q, d);
  quat_to_rot(q, R);
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) out_pose16[4 * c + r] = r == c ? 1.0 : 0.0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out_pose16[4 * j + i] = R[3 * i + j];
    out_pose16[12 + i] = d[i];
  }
  return NDT_OK;
}
