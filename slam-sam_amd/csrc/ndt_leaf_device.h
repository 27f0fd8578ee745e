// ndt_leaf_device.h -- the leaf rule: nine f64 moment sums of a voxel -> its statistics (internal; HIP).  One device
// function, finalize_leaf, shared by everything that turns sums into a Gaussian: the target builds and the map's target
// (ndt_target.hip) and the distribution source of the D2D registration (ndt_d2d.hip).  Whoever includes it is compiled
// with -ffp-contract=off like the rest of the engine, so a leaf has the same bits wherever it is made.
#pragma once

#include "ndt_kernels.h"

namespace ndt {

// one Jacobi rotation of the symmetric 3x3 A (full storage) in the (P,Q) plane
template <int P, int Q>
__device__ __forceinline__ void jacobi_rot(double A[9], double V[9]) {
  double apq = A[3 * P + Q];
  if (apq == 0.0) return;
  double theta = (A[3 * Q + Q] - A[3 * P + P]) / (2.0 * apq);
  double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double akp = A[3 * k + P], akq = A[3 * k + Q];
    A[3 * k + P] = c * akp - s * akq;
    A[3 * k + Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double apk = A[3 * P + k], aqk = A[3 * Q + k];
    A[3 * P + k] = c * apk - s * aqk;
    A[3 * Q + k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double vkp = V[3 * k + P], vkq = V[3 * k + Q];
    V[3 * k + P] = c * vkp - s * vkq;
    V[3 * k + Q] = s * vkp + c * vkq;
  }
}

#define NDT_SWAP_COL(a, b)                                          \
  {                                                                 \
    double td = d[a]; d[a] = d[b]; d[b] = td;                       \
    _Pragma("unroll") for (int k = 0; k < 3; ++k) {                 \
      double tv = V[3 * k + a]; V[3 * k + a] = V[3 * k + b]; V[3 * k + b] = tv; \
    }                                                               \
  }

// one leaf: count, cell, and its nine moment sums -> statistics, record, dense index entry
__device__ __forceinline__ bool finalize_leaf(int slot, int cell, int cnt, const double* __restrict__ in, FinalizeParams fp,
                                              VoxelRecord* __restrict__ rec, float4* __restrict__ cent,
                                              LeafStats* __restrict__ stats, int* __restrict__ cell2leaf) {
  const double s[3] = {in[0], in[1], in[2]};
  const double ss[6] = {in[3], in[4], in[5], in[6], in[7], in[8]};
  const double n = (double)cnt;
  double mean[3] = {s[0] / n, s[1] / n, s[2] / n};  // ref :278
  double C[9];
  const int tri[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
  if (fp.cov_mode == 0) {
    // ref :287-291
    const double k = n / (n - 1.0);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        C[3 * a + b] = ((ss[tri[3 * a + b]] / n) - (mean[a] * mean[b])) * k;
  } else {
    const double k = (n - 1.0) / n;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        C[3 * a + b] = ((ss[tri[3 * a + b]] - 2.0 * (s[a] * mean[b])) / n + mean[a] * mean[b]) * k;
  }

  LeafStats L;
  L.cell = cell;
  L.count = cnt;
#pragma unroll
  for (int a = 0; a < 3; ++a) L.mean[a] = mean[a];

  // eigen-decomposition (ref :298-300), cyclic Jacobi in f64
  double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
  for (int a = 0; a < 9; ++a) A[a] = C[a];
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
    double diag = A[0] * A[0] + A[4] * A[4] + A[8] * A[8];
    if (off <= 1e-32 * diag || off == 0.0) break;
    jacobi_rot<0, 1>(A, V);
    jacobi_rot<0, 2>(A, V);
    jacobi_rot<1, 2>(A, V);
  }
  double d[3] = {A[0], A[4], A[8]};
  if (d[0] > d[1]) NDT_SWAP_COL(0, 1);
  if (d[1] > d[2]) NDT_SWAP_COL(1, 2);
  if (d[0] > d[1]) NDT_SWAP_COL(0, 1);

  bool ok = !(d[0] < 0 || d[1] < 0 || d[2] < 1e-12);  // ref :303-309
  // ref :311-331
  const double floor_ev = fmax(1e-12, d[2] * fp.eig_ratio);
  bool recompose = false;
  if (d[0] < floor_ev) { d[0] = floor_ev; recompose = true; }
  if (d[1] < floor_ev) { d[1] = floor_ev; recompose = true; }
  if (recompose) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        double acc = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc += V[3 * a + k] * d[k] * V[3 * b + k];
        C[3 * a + b] = acc;
      }
  }
  // inverse by cofactors (ref :334)
  double c00 = C[4] * C[8] - C[5] * C[7];
  double c01 = C[5] * C[6] - C[3] * C[8];
  double c02 = C[3] * C[7] - C[4] * C[6];
  double det = C[0] * c00 + C[1] * c01 + C[2] * c02;
  double id = 1.0 / det;
  double I[9];
  I[0] = c00 * id;
  I[1] = (C[2] * C[7] - C[1] * C[8]) * id;
  I[2] = (C[1] * C[5] - C[2] * C[4]) * id;
  I[3] = c01 * id;
  I[4] = (C[0] * C[8] - C[2] * C[6]) * id;
  I[5] = (C[2] * C[3] - C[0] * C[5]) * id;
  I[6] = c02 * id;
  I[7] = (C[1] * C[6] - C[0] * C[7]) * id;
  I[8] = (C[0] * C[4] - C[1] * C[3]) * id;
  double amax = 0;
#pragma unroll
  for (int a = 0; a < 9; ++a) {
    if (!isfinite(I[a])) ok = false;
    amax = fmax(amax, fabs(I[a]));
  }
  if (amax > 1e12) ok = false;  // ref :337-343

#pragma unroll
  for (int a = 0; a < 9; ++a) { L.cov[a] = C[a]; L.icov[a] = I[a]; L.evecs[a] = V[a]; }
#pragma unroll
  for (int a = 0; a < 3; ++a) L.evals[a] = d[a];
  if (!ok) L.count = -cnt;
  stats[slot] = L;
  // Every slot gets a finite record: the derivative kernel reads record 0 for an absent
  // neighbour (masked by f = 0, but 0 * NaN would still poison the sums), and slot 0 may well be
  // a rejected leaf.  Only accepted leaves are reachable through the cell -> leaf grid.
  VoxelRecord r;
  r.mean[0] = ok ? mean[0] : 0.0; r.mean[1] = ok ? mean[1] : 0.0; r.mean[2] = ok ? mean[2] : 0.0;
  r.icov[0] = ok ? I[0] : 0.0; r.icov[1] = ok ? I[1] : 0.0; r.icov[2] = ok ? I[2] : 0.0;
  r.icov[3] = ok ? I[4] : 0.0; r.icov[4] = ok ? I[5] : 0.0; r.icov[5] = ok ? I[8] : 0.0;
  r.pad = (double)cnt;
  rec[slot] = r;
  // the centroid as the radius search sees it (f32-rounded leaf mean, ref: voxel_grid_covariance_impl.hpp:420-422),
  // 16 bytes per leaf: the KDTREE / multi-grid neighbourhoods test 27 cells per point against it; w = "no further leaf
  // in this cell" (the multi-grid union chains leaves through it)
  cent[slot] = make_float4((float)r.mean[0], (float)r.mean[1], (float)r.mean[2], __int_as_float(-1));
  if (ok) cell2leaf[cell] = slot;
  return ok;
}

}  // namespace ndt
