// ndt_deskew_device.h -- what the kernels of ndt_deskew.hip and ndt_unproject.hip share (internal; HIP): the acquisition
// filter's predicate, the block's copy of the knot table and the motion of one point, plus the overlap check their host
// sides have in common.  One definition each: the unprojection's contract is bit equality with ndt_deskew_device on the
// same points.  The layout rule of a host cloud is in ndt_host_cloud.h.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "../../include/ndt_hip.h"
#include "ndt_trajectory.h"

namespace ndt {

constexpr int DSK_THREADS = 256, DSK_WAVES = DSK_THREADS / 64;

// the acquisition filter on the RAW point (sensor frame), every comparison inclusive as the header states it
__device__ __forceinline__ bool dsk_keep(const ndt_scan_filter& f, float x, float y, float z, float t, const float* intensity,
                                         size_t i) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z) && isfinite(t))) return false;
  if (f.use_box && f.box_min[0] <= x && x <= f.box_max[0] && f.box_min[1] <= y && y <= f.box_max[1] && f.box_min[2] <= z &&
      z <= f.box_max[2])
    return false;
  if (!f.use_z_or_intensity) return true;
  if (f.z_min <= z && z <= f.z_max) return true;
  return intensity != nullptr && intensity[i] >= f.intensity_keep_min;
}

// the block's copy of the knot table
__device__ __forceinline__ void dsk_load_table(const double* __restrict__ table, int n_knots, double* s_tab) {
  for (int w = (int)threadIdx.x; w < n_knots * traj::ROW_WORDS; w += DSK_THREADS) s_tab[w] = table[w];
  __syncthreads();
}

// p' = R(q(u)) p + d(u) in f64, rounded to f32 once; the exact identity hands the point back as it is
__device__ __forceinline__ void dsk_move(const traj::KnotRow* rows, int n_knots, float x, float y, float z, float t, float* ox,
                                         float* oy, float* oz) {
  double q[4], d[3], R[9];
  if (traj::pose_at(rows, n_knots, (double)t, q, d)) {
    *ox = x; *oy = y; *oz = z;
    return;
  }
  traj::quat_to_rot(q, R);
  const double px = (double)x, py = (double)y, pz = (double)z;
  *ox = (float)(R[0] * px + R[1] * py + R[2] * pz + d[0]);
  *oy = (float)(R[3] * px + R[4] * py + R[5] * pz + d[1]);
  *oz = (float)(R[6] * px + R[7] * py + R[8] * pz + d[2]);
}

namespace engine {

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || na == 0 || nb == 0) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

}  // namespace engine
}  // namespace ndt
