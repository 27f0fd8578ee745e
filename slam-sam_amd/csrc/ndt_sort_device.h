// ndt_sort_device.h -- what the kernels that feed or mirror the radix sort share with it (internal; HIP): the tile shape
// and its order, and the wave scan.  The sort itself is ndt_sort.hip; k_cell_keys, k_sort_pass, k_source_keys and the
// bucketed build (ndt_target.hip) count a first digit or rank a tile in the same shape.
#pragma once

#include <hip/hip_runtime.h>

namespace ndt {

// ---- stable LSD radix sort of (cell key, point index) ---------------------------------
// One tile = 2048 consecutive pairs per 256-thread block; wave w owns the contiguous
// quarter [w*512, (w+1)*512) of the tile and walks it in 8 rounds of 64, so "tile order"
// is (wave, round, lane).  Per digit pass: count (per-tile histogram, bin-major), scan (one
// block per bin over the tiles + bin totals), scatter (rank of a pair among the equal
// digits before it in the tile: equal-digit lanes of a round find each other with 8
// ballots, rounds chain through a per-wave LDS counter, waves through a 4-entry prefix).
// No atomics on global memory, no look-back chain between tiles: every launch is a
// streaming pass, and the result does not depend on scheduling.
constexpr int SORT_THREADS = 256;
constexpr int SORT_ROUNDS = 8;
constexpr int SORT_WAVES = SORT_THREADS / 64;
constexpr int SORT_TILE = SORT_THREADS * SORT_ROUNDS;
constexpr int SORT_BINS = 256;
// (Round 2 tried to let scatter pass p count the tile histogram of pass p + 1 with integer atomics
// on a global table -- one launch per pass less.  A million device-scope atomicAdds spread over
// 125 k counters took 88-248 us per pass: across eight XCDs they are served at the memory side.
// Reverted; the per-tile LDS histogram of k_sort_count costs 6 us.)

__device__ __forceinline__ int sort_index(int tile, int wave, int round, int lane) {
  return tile * SORT_TILE + wave * (SORT_TILE / SORT_WAVES) + round * 64 + lane;
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    int t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

}  // namespace ndt
