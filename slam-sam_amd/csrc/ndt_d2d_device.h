// ndt_d2d_device.h -- one pair of Gaussians under a pose (internal; HIP): q = mu^T (R Sigma_i R^T + Sigma_j)^-1 mu and
// its exact first and second derivatives by the six pose parameters, as include/ndt_hip.h states them for
// ndt_eval_derivatives_d2d.  Three evaluations share it and differ only in the WEIGHT a pair's q enters the sums with:
//   D2dNdtWeight   distribution-to-distribution NDT (ndt_d2d.hip): score -d1 exp(-d2 q / 2), f = (d1 d2 / 2) e
//   D2dHalfWeight  GICP's plane-to-plane cost (ndt_gicp.hip): score -q / 2, f = -1/2, no q_a q_b term
//   D2dCountWeight voxelised GICP (ndt_vgicp.hip): the partner is a voxel of N points, score -N q / 2, f = -N / 2, no q_a q_b term
// Also here: the pose's rotation with its angle derivatives (host side) and the small symmetric-matrix helpers.
// Whoever includes it is compiled with -ffp-contract=off like the rest of the engine.
#pragma once

#include <cmath>
#include <cstring>

#include "ndt_kernels.h"

namespace ndt {

// R = Rx(roll) Ry(pitch) Rz(yaw) and its first and second angle derivatives, row-major, f64 from exact sin / cos
struct D2dPose {
  double R[9];
  double dR[3][9];    // by roll, pitch, yaw
  double d2R[6][9];   // rr, rp, ry, pp, py, yy
  double t[3];
};

struct Sym3 {
  double xx, xy, xz, yy, yz, zz;
};

__device__ __forceinline__ void sym_mul(const Sym3& S, const double v[3], double o[3]) {
  o[0] = (S.xx * v[0] + S.xy * v[1]) + S.xz * v[2];
  o[1] = (S.xy * v[0] + S.yy * v[1]) + S.yz * v[2];
  o[2] = (S.xz * v[0] + S.yz * v[1]) + S.zz * v[2];
}
__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void mat_vec(const double* A, const double v[3], double o[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = (A[3 * a] * v[0] + A[3 * a + 1] * v[1]) + A[3 * a + 2] * v[2];
}
// M = A S B^T (A, B row-major 3 x 3, S symmetric)
__device__ __forceinline__ void a_s_bt(const double* A, const Sym3& S, const double* B, double M[9]) {
  double T[9];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    T[3 * a + 0] = (A[3 * a] * S.xx + A[3 * a + 1] * S.xy) + A[3 * a + 2] * S.xz;
    T[3 * a + 1] = (A[3 * a] * S.xy + A[3 * a + 1] * S.yy) + A[3 * a + 2] * S.yz;
    T[3 * a + 2] = (A[3 * a] * S.xz + A[3 * a + 1] * S.yz) + A[3 * a + 2] * S.zz;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) M[3 * a + b] = (T[3 * a] * B[3 * b] + T[3 * a + 1] * B[3 * b + 1]) + T[3 * a + 2] * B[3 * b + 2];
}
// M + M^T
__device__ __forceinline__ Sym3 sym_of(const double M[9]) {
  Sym3 Z;
  Z.xx = M[0] + M[0]; Z.xy = M[1] + M[3]; Z.xz = M[2] + M[6];
  Z.yy = M[4] + M[4]; Z.yz = M[5] + M[7]; Z.zz = M[8] + M[8];
  return Z;
}
// sum_ab Z_ab W_ab of two symmetric matrices
__device__ __forceinline__ double sym_inner(const Sym3& Z, const Sym3& W) {
  return ((Z.xx * W.xx + Z.yy * W.yy) + Z.zz * W.zz) + 2.0 * ((Z.xy * W.xy + Z.xz * W.xz) + Z.yz * W.yz);
}

// The weight of a pair: weigh(q, &score, &f) says whether the pair counts and with which score and factor f it enters
// gradient and Hessian; QQ: the Hessian carries -(qq() f) q_a q_b beside f q_ab.
struct D2dNdtWeight {
  double d1, d2;
  static constexpr bool QQ = true;
  __device__ __forceinline__ bool weigh(double q, double* sc, double* f) const {
    const double e = exp(-d2 * q * 0.5);
    if (!(e >= 0.0 && e <= 1.0)) return false;   // the evaluation's guard (a NaN fails both compares)
    *sc = -d1 * e;
    *f = (d1 * d2 * 0.5) * e;
    return true;
  }
  __device__ __forceinline__ double qq() const { return 0.5 * d2; }
};
struct D2dHalfWeight {
  static constexpr bool QQ = false;
  __device__ __forceinline__ bool weigh(double q, double* sc, double* f) const {
    if (!isfinite(q)) return false;
    *sc = -0.5 * q;
    *f = -0.5;
    return true;
  }
  __device__ __forceinline__ double qq() const { return 0.0; }
};

struct D2dCountWeight {
  double n;   // (double)N of the voxel
  static constexpr bool QQ = false;
  __device__ __forceinline__ bool weigh(double q, double* sc, double* f) const {
    if (!isfinite(q)) return false;
    *f = -0.5 * n;
    *sc = *f * q;
    return true;
  }
  __device__ __forceinline__ double qq() const { return 0.0; }
};

// What a lane keeps over its pairs.  The Hessian's terms that are linear in a pair's f v and f v v^T (v = B mu) are
// summed as w and W and meet the second derivatives of the pose once per lane, behind the pairs (d2d_second_order):
//   q_ab = 2 u_b^T B u_a + 2 v^T H_ab - v^T Z_ab v,   u_a = j_a - Z_a v,   q_a = v^T (j_a + u_a)
// (the six products of the rule's q_ab in j, Z, B and v fold into u_b^T B u_a).
template <bool HESSIAN>
struct D2dAcc {
  double score, best;
  int npairs;
  double g[6];
  double H[HESSIAN ? 21 : 1];
  double w[3];
  Sym3 W;
};

template <bool HESSIAN>
__device__ __forceinline__ void d2d_acc_clear(D2dAcc<HESSIAN>& acc) {
  acc.score = 0.0; acc.best = 0.0; acc.npairs = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) acc.g[a] = 0.0;
#pragma unroll
  for (int a = 0; a < (HESSIAN ? 21 : 1); ++a) acc.H[a] = 0.0;
  acc.w[0] = acc.w[1] = acc.w[2] = 0.0;
  acc.W.xx = acc.W.xy = acc.W.xz = acc.W.yy = acc.W.yz = acc.W.zz = 0.0;
}

// what depends on the pose and the source Gaussian alone: A = R S R^T, j_c = (dR_c) mu, Z_c = (dR_c) S R^T + transpose
__device__ __forceinline__ void d2d_source_terms(const D2dPose& P, const double mu[3], const Sym3& S, Sym3& A, double (&j)[3][3],
                                                 Sym3 (&Z)[3]) {
  double M[9];
  a_s_bt(P.R, S, P.R, M);
  A.xx = M[0]; A.xy = M[1]; A.xz = M[2]; A.yy = M[4]; A.yz = M[5]; A.zz = M[8];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    mat_vec(P.dR[c], mu, j[c]);
    a_s_bt(P.dR[c], S, P.R, M);
    Z[c] = sym_of(M);
  }
}

// one pair: the source Gaussian moved to m with A = R S R^T against the target Gaussian T = {mean 3, cov xx xy xz yy yz zz}
template <bool HESSIAN, typename Weight>
__device__ __forceinline__ void d2d_pair(D2dAcc<HESSIAN>& acc, const double* __restrict__ T, const double m[3], const Sym3& A,
                                         const double (&j)[3][3], const Sym3 (&Z)[3], const Weight& wt) {
  const double mu[3] = {m[0] - T[0], m[1] - T[1], m[2] - T[2]};
  Sym3 C;
  C.xx = A.xx + T[3]; C.xy = A.xy + T[4]; C.xz = A.xz + T[5]; C.yy = A.yy + T[6]; C.yz = A.yz + T[7]; C.zz = A.zz + T[8];
  // B = C^-1 by cofactors
  const double c00 = C.yy * C.zz - C.yz * C.yz;
  const double c01 = C.xz * C.yz - C.xy * C.zz;
  const double c02 = C.xy * C.yz - C.xz * C.yy;
  const double det = (C.xx * c00 + C.xy * c01) + C.xz * c02;
  const double id = 1.0 / det;
  Sym3 B;
  B.xx = c00 * id; B.xy = c01 * id; B.xz = c02 * id;
  B.yy = (C.xx * C.zz - C.xz * C.xz) * id;
  B.yz = (C.xy * C.xz - C.xx * C.yz) * id;
  B.zz = (C.xx * C.yy - C.xy * C.xy) * id;
  double v[3];
  sym_mul(B, mu, v);
  const double q = dot3(mu, v);
  double sc, f;
  if (!wt.weigh(q, &sc, &f)) return;
  acc.score += sc;
  acc.best = fmax(acc.best, sc);
  acc.npairs += 1;
  double u[3][3], qa[6];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double zv[3];
    sym_mul(Z[c], v, zv);
#pragma unroll
    for (int a = 0; a < 3; ++a) u[c][a] = j[c][a] - zv[a];
    const double ju[3] = {j[c][0] + u[c][0], j[c][1] + u[c][1], j[c][2] + u[c][2]};
    qa[c] = 2.0 * v[c];
    qa[3 + c] = dot3(v, ju);
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) acc.g[a] += f * qa[a];
  if (HESSIAN) {
    // B u_a: the columns of B for the translations, then the three rotations
    double Bu[6][3] = {{B.xx, B.xy, B.xz}, {B.xy, B.yy, B.yz}, {B.xz, B.yz, B.zz}};
#pragma unroll
    for (int c = 0; c < 3; ++c) sym_mul(B, u[c], Bu[3 + c]);
    const double hd = wt.qq();
    int w = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) {
        // u_b^T B u_a (u of a translation is a unit vector)
        const double ubu = b < 3 ? Bu[a][b] : dot3(u[b - 3], Bu[a]);
        if (Weight::QQ) acc.H[w] += f * (2.0 * ubu - hd * qa[a] * qa[b]);
        else acc.H[w] += f * (2.0 * ubu);
        ++w;
      }
    acc.w[0] += f * v[0]; acc.w[1] += f * v[1]; acc.w[2] += f * v[2];
    acc.W.xx += f * v[0] * v[0]; acc.W.xy += f * v[0] * v[1]; acc.W.xz += f * v[0] * v[2];
    acc.W.yy += f * v[1] * v[1]; acc.W.yz += f * v[1] * v[2]; acc.W.zz += f * v[2] * v[2];
  }
}

// behind a lane's pairs: the rotation block's second-derivative terms 2 w^T H_cd - <Z_cd, W>, Z_cd = N + N^T,
// N = (d2R_cd) S R^T + (dR_c) S (dR_d)^T
__device__ __forceinline__ void d2d_second_order(D2dAcc<true>& acc, const D2dPose& P, const double mu[3], const Sym3& S) {
  int q = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int d = c; d < 3; ++d) {
      double hcd[3], N[9], N2[9];
      mat_vec(P.d2R[q], mu, hcd);
      a_s_bt(P.d2R[q], S, P.R, N);
      a_s_bt(P.dR[c], S, P.dR[d], N2);
#pragma unroll
      for (int a = 0; a < 9; ++a) N[a] += N2[a];
      const Sym3 Zcd = sym_of(N);
      // word of (3 + c, 3 + d) in the upper triangle row by row: rows 0 .. 2 hold 6 + 5 + 4 = 15 words
      const int word = 15 + (c == 0 ? d : c == 1 ? 3 + (d - 1) : 5);
      acc.H[word] += 2.0 * dot3(acc.w, hcd) - sym_inner(Zcd, acc.W);
      ++q;
    }
}
__device__ __forceinline__ void d2d_second_order(D2dAcc<false>&, const D2dPose&, const double*, const Sym3&) {}

// a lane's sums as the EV_WORDS of eval_block_row (word 31 = 0); nvtl: what goes into EV_NVTL
template <bool HESSIAN>
__device__ __forceinline__ void d2d_words(const D2dAcc<HESSIAN>& acc, double nvtl, double* words) {
  words[EV_SCORE] = acc.score;
#pragma unroll
  for (int a = 0; a < 6; ++a) words[EV_G + a] = acc.g[a];
#pragma unroll
  for (int a = 0; a < 21; ++a) words[EV_H + a] = HESSIAN ? acc.H[a] : 0.0;
  words[EV_NVTL] = nvtl;
  words[EV_NWITH] = acc.npairs > 0 ? 1.0 : 0.0;
  words[EV_NPAIRS] = (double)acc.npairs;
  words[EV_FAIL] = 0.0;
}

// ---- host side: the pose's rotation and its angle derivatives ----
inline void rot_axis(char axis, double a, int order, double M[9]) {   // order-th derivative of Rx / Ry / Rz (a)
  const double s = std::sin(a), c = std::cos(a);
  const double f[3][2] = {{c, s}, {-s, c}, {-c, -s}};   // {cos, sin} and their derivatives
  const double C = f[order][0], Sn = f[order][1], one = order == 0 ? 1.0 : 0.0;
  const double mx[9] = {one, 0, 0, 0, C, -Sn, 0, Sn, C};
  const double my[9] = {C, 0, Sn, 0, one, 0, -Sn, 0, C};
  const double mz[9] = {C, -Sn, 0, Sn, C, 0, 0, 0, one};
  std::memcpy(M, axis == 'x' ? mx : axis == 'y' ? my : mz, sizeof(mx));
}
inline void mul3(const double* A, const double* B, double* C) {
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) C[3 * a + b] = (A[3 * a] * B[b] + A[3 * a + 1] * B[3 + b]) + A[3 * a + 2] * B[6 + b];
}
// (d/droll)^o0 (d/dpitch)^o1 (d/dyaw)^o2 of Rx Ry Rz
inline void rot_product(const double p[6], int o0, int o1, int o2, double M[9]) {
  double X[9], Y[9], Zm[9], XY[9];
  rot_axis('x', p[3], o0, X);
  rot_axis('y', p[4], o1, Y);
  rot_axis('z', p[5], o2, Zm);
  mul3(X, Y, XY);
  mul3(XY, Zm, M);
}
inline void fill_d2d_pose(const double p[6], D2dPose* P) {
  rot_product(p, 0, 0, 0, P->R);
  rot_product(p, 1, 0, 0, P->dR[0]);
  rot_product(p, 0, 1, 0, P->dR[1]);
  rot_product(p, 0, 0, 1, P->dR[2]);
  rot_product(p, 2, 0, 0, P->d2R[0]);
  rot_product(p, 1, 1, 0, P->d2R[1]);
  rot_product(p, 1, 0, 1, P->d2R[2]);
  rot_product(p, 0, 2, 0, P->d2R[3]);
  rot_product(p, 0, 1, 1, P->d2R[4]);
  rot_product(p, 0, 0, 2, P->d2R[5]);
  for (int a = 0; a < 3; ++a) P->t[a] = p[a];
}

}  // namespace ndt
