// ndt_neighbors_device.h -- which voxels a moved point pairs with (internal; HIP).  THE statement of the rule for every
// evaluator: the hot kernel's phase 1 (point_pairs / point_pairs_kd) and k_point_scores (ndt_derivs.hip), k_d2d_eval
// (ndt_d2d.hip) and k_ct_eval (ndt_ct.hip) all call the functions below, so a point on a voxel face has the same
// neighbours in ndt_score_points as in the align that scored it.  Whoever includes it is compiled with
// -ffp-contract=off like the rest of the engine: the transform and the index arithmetic must round exactly as written
// to classify points into the same voxels as the reference.
//
// Classifying a point into a voxel (ref: voxel_grid_covariance_impl.hpp:46-71 for the f32 bounds
// test, voxel_grid_covariance.h:297-300 for the index):
//   in   = lo <= p < hi on every axis (f32);   i_a = (int)(floorf(p_a * inv_leaf) - (float)min_b_a);
//   idx  = i0 + i1 * mul1 + i2 * mul2.
// The reference looks idx up in its hash map whatever its value (f32 rounding at an upper face
// can alias into the next row); an idx outside [0, ncells) can never be a stored key there, so
// it is a miss here too -- same outcome.  neighbor_cells7() evaluates this for the point and its
// six face-offset copies with the per-axis pieces shared.
#pragma once

#include "ndt_device.h"

namespace ndt {

// x' = r0*x + (r1*y + (r2*z + t)), f32, unfused (transformPointCloud, ref :761).  RT: anything with R[9] and t[3].
template <class RT>
__device__ __forceinline__ void rigid_apply(const RT& P, float x, float y, float z, float& xt, float& yt, float& zt) {
  xt = P.R[0] * x + (P.R[1] * y + (P.R[2] * z + P.t[0]));
  yt = P.R[3] * x + (P.R[4] * y + (P.R[5] * z + P.t[1]));
  zt = P.R[6] * x + (P.R[7] * y + (P.R[8] * z + P.t[2]));
}

// The moved point of a lane; false: the lane has no point (active = false) or the moved point is not finite (ref :573:
// such points are skipped).  Either comes back as the origin, which keeps NaN / Inf out of the index casts and of the
// (masked) pair arithmetic -- it has no neighbours.
template <class RT>
__device__ __forceinline__ bool rigid_move(const RT& P, float x, float y, float z, bool active, float& xt, float& yt, float& zt) {
  rigid_apply(P, x, y, z, xt, yt, zt);
  const bool finite = active && isfinite(xt) && isfinite(yt) && isfinite(zt);
  if (!finite) { xt = 0.0f; yt = 0.0f; zt = 0.0f; }
  return finite;
}

// The cells of the point's own voxel and of its six face neighbours, in the pair order 0, +x, -x, +y, -y, +z, -z; -1: no
// such cell.  D7 = false (DIRECT1, ref: getNeighborhoodAtPoint1, voxel_grid_covariance_impl.hpp:604-615): cell[0] only,
// the rest -1.
// ref: voxel_grid_covariance_impl.hpp:560-600 -- neighbours are found by offsetting the
// POINT by +-leaf in f32 and re-classifying it (see above).  The seven classifications share
// their per-axis pieces: a probe differs from the centre in one coordinate only, so only that
// axis' bounds test, floor and index are recomputed -- same f32 operations on the same
// operands as seven independent classifications, a third of the instructions.
// (The `if (D7) ... else` shape is the one k_derivatives was scheduled and measured with: folding D7 into the
// conditions compiles to a different instruction stream there.)
template <bool D7>
__device__ __forceinline__ void neighbor_cells7(float xt, float yt, float zt, const GridGeom& g, int (&cell)[7]) {
  const float w = g.leaf;
  const float cx[3] = {xt, xt + w, xt - w}, cy[3] = {yt, yt + w, yt - w}, cz[3] = {zt, zt + w, zt - w};
  bool inx[3], iny[3], inz[3];
  unsigned int ix[3], iy[3], iz[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    inx[k] = cx[k] >= g.lo[0] && cx[k] < g.hi[0];
    iny[k] = cy[k] >= g.lo[1] && cy[k] < g.hi[1];
    inz[k] = cz[k] >= g.lo[2] && cz[k] < g.hi[2];
    // (out-of-range coordinates convert to saturated garbage that the bounds flags mask;
    // unsigned arithmetic so that garbage may wrap)
    ix[k] = (unsigned int)(int)(floorf(cx[k] * g.inv_leaf) - (float)g.min_b[0]);
    iy[k] = (unsigned int)(int)(floorf(cy[k] * g.inv_leaf) - (float)g.min_b[1]) * (unsigned int)g.mul1;
    iz[k] = (unsigned int)(int)(floorf(cz[k] * g.inv_leaf) - (float)g.min_b[2]) * (unsigned int)g.mul2;
  }
  {
    const int idx0 = (int)(ix[0] + iy[0] + iz[0]);
    cell[0] = (inx[0] && iny[0] && inz[0] && idx0 >= 0 && idx0 < g.ncells) ? idx0 : -1;
  }
  if (D7) {
#pragma unroll
    for (int k = 1; k < 3; ++k) {
      const int ax = (int)(ix[k] + iy[0] + iz[0]), ay = (int)(ix[0] + iy[k] + iz[0]), az = (int)(ix[0] + iy[0] + iz[k]);
      // an idx outside [0, ncells) can never be a stored key of the reference's hash map: a miss
      cell[k] = (inx[k] && iny[0] && inz[0] && ax >= 0 && ax < g.ncells) ? ax : -1;
      cell[2 + k] = (inx[0] && iny[k] && inz[0] && ay >= 0 && ay < g.ncells) ? ay : -1;
      cell[4 + k] = (inx[0] && iny[0] && inz[k] && az >= 0 && az < g.ncells) ? az : -1;
    }
  } else {
#pragma unroll
    for (int k = 1; k < 7; ++k) cell[k] = -1;
  }
}

// cell -> leaf slot (-1: no leaf, no cell, or a point that is not finite) for the cells a neighbourhood has
template <bool D7>
__device__ __forceinline__ void neighbor_slots7(const int (&cell)[7], bool finite, const int* __restrict__ cell2leaf,
                                                int (&slot)[7]) {
#pragma unroll
  for (int k = 0; k < (D7 ? 7 : 1); ++k) slot[k] = (finite && cell[k] >= 0) ? cell2leaf[cell[k]] : -1;
}

// What is NOT here.  The 27-cell lookup of KDTREE / DIRECT26 / the multi-grid union (nine masked 12-byte row loads) stays
// written out in its two users, point_pairs_kd and k_point_scores (ndt_derivs.hip), and point_pairs keeps the one-line
// gather of neighbor_slots7 written out as well.  Every shape of a shared helper that was tried for them -- a struct of
// the row flags, reference outputs of the original types, a per-row callback, a one-slot function -- left the results
// alone but changed the scalar-register count or the schedule of k_derivatives instantiations that are tuned and
// measured as they stand (profiles/neighbours_refactor_resources.txt).  neighbor_cells7 in point_pairs costs DIRECT1 three
// swapped instruction pairs and DIRECT7 two instructions, with every resource number unchanged.

}  // namespace ndt
