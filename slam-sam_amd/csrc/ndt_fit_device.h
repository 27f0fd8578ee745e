// ndt_fit_device.h -- the device side of the point-level nearest-neighbour index (internal; HIP): cell hash, cell
// classification, the table lookup, the query's place in the grid, the conservative lower bound on everything a scanned
// box leaves out, and the walk over a box and over the Chebyshev shells around it.  The index itself is built by
// fit_build_cloud (ndt_fitness.hip) over any SoA cloud; getFitnessScore (ndt_fitness.hip) and GICP's neighbour search
// and pairing (ndt_gicp.hip) query it through the functions below, so a point on a cell face is classified the same
// way everywhere and every query stops on the same bound.
#pragma once

#include "ndt_engine.h"

namespace ndt {
namespace engine {

constexpr uint32_t FIT_EMPTY = 0xffffffffu;

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z);
}

// (murmur3's finaliser: neighbouring cells -- keys that differ by 1, dims0 or dims0 * dims1 -- land far apart)
__device__ __forceinline__ uint32_t fit_hash(uint32_t key, uint32_t mask) {
  key ^= key >> 16; key *= 0x85ebca6bu; key ^= key >> 13; key *= 0xc2b2ae35u; key ^= key >> 16;
  return key & mask;
}

// cell coordinate of u = (p - lo) * inv_c on one axis, clamped to [-1, dims] (a point outside the box searches from
// the box's face; the lower bounds below use u itself, so the clamp never costs exactness)
__device__ __forceinline__ int fit_cell(float u, int dims) {
  const float f = fminf(fmaxf(floorf(u), -1.0f), (float)dims);
  return (int)f;
}

__device__ __forceinline__ uint32_t fit_key(const FitGeom& g, int cx, int cy, int cz) {
  return (uint32_t)cx + (uint32_t)g.dims[0] * ((uint32_t)cy + (uint32_t)g.dims[1] * (uint32_t)cz);
}

__device__ __forceinline__ int fit_find(const uint4* __restrict__ tab, uint32_t mask, uint32_t key, uint32_t* first,
                                        uint32_t* end) {
  uint32_t slot = fit_hash(key, mask);
  for (;;) {
    const uint4 e = tab[slot];
    if (e.x == key) { *first = e.y; *end = e.z; return 1; }
    if (e.x == FIT_EMPTY) return 0;
    slot = (slot + 1) & mask;
  }
}

struct FitQuery {
  float qx, qy, qz;    // the query point
  float u[3];          // (q - lo) * inv_c
  int k[3];            // its cell, clamped to [-1, dims]
};

// u and k of a finite query point whose qx / qy / qz are set
__device__ __forceinline__ void fit_locate(const FitGeom& g, FitQuery* q) {
  q->u[0] = (q->qx - g.lo[0]) * g.inv_c;
  q->u[1] = (q->qy - g.lo[1]) * g.inv_c;
  q->u[2] = (q->qz - g.lo[2]) * g.inv_c;
#pragma unroll
  for (int a = 0; a < 3; ++a) q->k[a] = fit_cell(q->u[a], g.dims[a]);
}

// Squared lower bound on the distance from q to any indexed point in a cell OUTSIDE the scanned box
// [k - r, k + r]^3 (clipped to the grid); +INF when the scanned box covers the grid.  A point of such a cell lies
// beyond one face of the scanned box on some axis a (gap_a) and inside the bounding box on every axis (dG_b), so its
// distance is at least sqrt(max(gap_a, dG_a)^2 + sum_{b != a} dG_b^2); the bound is the minimum over the faces that
// still have cells behind them.  Everything is in cell units, shrunk by a slack that covers the f32 rounding of the
// cell classification (relative ~1.2e-7 of |u|, on the indexed points' side and on the query's) and of d^2 itself, so a
// closer point can never hide behind a mis-classified cell at km-scale coordinates.
__device__ __forceinline__ float fit_lower_bound2(const FitQuery& q, const FitGeom& g, int r) {
  float dG[3], slack[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    slack[a] = 1e-6f * (fabsf(q.u[a]) + (float)g.dims[a] + (float)r + 2.0f);
    dG[a] = fmaxf(fmaxf(-q.u[a], q.u[a] - (float)g.dims[a]) - slack[a], 0.0f);
  }
  const float s2 = dG[0] * dG[0] + dG[1] * dG[1] + dG[2] * dG[2];
  float lb2 = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float rest = s2 - dG[a] * dG[a];
    if (q.k[a] - r > 0) {
      const float gap = fmaxf(fmaxf(q.u[a] - (float)(q.k[a] - r) - slack[a], dG[a]), 0.0f);
      lb2 = fminf(lb2, fmaxf(rest, 0.0f) + gap * gap);
    }
    if (q.k[a] + r < g.dims[a] - 1) {
      const float gap = fmaxf(fmaxf((float)(q.k[a] + r + 1) - q.u[a] - slack[a], dG[a]), 0.0f);
      lb2 = fminf(lb2, fmaxf(rest, 0.0f) + gap * gap);
    }
  }
  return lb2 * (g.c * g.c) * (1.0f - 4e-6f);
}

// the largest shell radius a walk can need
__device__ __forceinline__ int fit_rmax(const FitGeom& g) { return max(g.dims[0], max(g.dims[1], g.dims[2])) + 1; }

// visit(cx, cy, cz) for every grid cell of the box [k - 1, k + 1]^3, z-major
template <typename F>
__device__ __forceinline__ void fit_walk_box(const FitQuery& q, const FitGeom& g, F&& visit) {
  const int z0 = max(q.k[2] - 1, 0), z1 = min(q.k[2] + 1, g.dims[2] - 1);
  const int y0 = max(q.k[1] - 1, 0), y1 = min(q.k[1] + 1, g.dims[1] - 1);
  const int x0 = max(q.k[0] - 1, 0), x1 = min(q.k[0] + 1, g.dims[0] - 1);
  for (int cz = z0; cz <= z1; ++cz)
    for (int cy = y0; cy <= y1; ++cy)
      for (int cx = x0; cx <= x1; ++cx) visit(cx, cy, cz);
}

// visit(cx, cy, cz) for every grid cell of the Chebyshev shell r >= 2 around k, clipped to the grid
template <typename F>
__device__ __forceinline__ void fit_walk_shell(const FitQuery& q, const FitGeom& g, int r, F&& visit) {
  const int z0 = max(q.k[2] - r, 0), z1 = min(q.k[2] + r, g.dims[2] - 1);
  const int y0 = max(q.k[1] - r, 0), y1 = min(q.k[1] + r, g.dims[1] - 1);
  const int x0 = max(q.k[0] - r, 0), x1 = min(q.k[0] + r, g.dims[0] - 1);
  for (int cz = z0; cz <= z1; ++cz) {
    const bool zface = cz == q.k[2] - r || cz == q.k[2] + r;
    for (int cy = y0; cy <= y1; ++cy) {
      if (zface || cy == q.k[1] - r || cy == q.k[1] + r) {
        for (int cx = x0; cx <= x1; ++cx) visit(cx, cy, cz);
      } else {
        if (q.k[0] - r >= 0) visit(q.k[0] - r, cy, cz);
        if (q.k[0] + r <= g.dims[0] - 1) visit(q.k[0] + r, cy, cz);
      }
    }
  }
}

}  // namespace engine
}  // namespace ndt
