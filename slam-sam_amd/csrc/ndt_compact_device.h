// ndt_compact_device.h -- the stable stream compaction every "keep what passes, in input order" kernel pair shares
// (internal; HIP).  A count kernel and an emit kernel evaluate the same predicate, one element per thread:
//   count   compact_ballot -> barrier -> compact_block_count                       counts[block] = kept by the block
//   scan    k_filter_scan (launch_filter_scan, ndt_point_scores.hip), one block    counts -> exclusive offsets + total
//   emit    compact_ballot -> barrier -> compact_position                          where a kept element lands
// The helpers take the kernel's own __shared__ word per wave and leave the barrier to the kernel, which may have one
// already (a table load's).  Whether a position is written is the kernel's rule (pos < cap).  Integer counters only, no
// atomics.  The host side of a compaction is CompactBufs / compact_total (ndt_engine.h).
#pragma once

#include <hip/hip_runtime.h>

namespace ndt {

// the wave's ballot of `keep`; lane 0 stores its popcount to s_w[wave] for the barrier that follows
template <int WAVES>
__device__ __forceinline__ unsigned long long compact_ballot(bool keep, unsigned int (&s_w)[WAVES]) {
  const unsigned long long bal = __ballot(keep);
  if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = (unsigned int)__popcll(bal);
  return bal;
}

// behind the barrier: counts[blockIdx.x] = what the block keeps
template <int WAVES>
__device__ __forceinline__ void compact_block_count(const unsigned int (&s_w)[WAVES], unsigned int* __restrict__ counts) {
  if (threadIdx.x == 0) {
    unsigned int c = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) c += s_w[w];
    counts[blockIdx.x] = c;
  }
}

// behind the barrier: the block's offset + the waves in front of this one + the kept lanes in front of this one
template <int WAVES>
__device__ __forceinline__ unsigned int compact_position(unsigned long long bal, const unsigned int (&s_w)[WAVES],
                                                         const unsigned int* __restrict__ offsets) {
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  unsigned int wave_off = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) wave_off += w < wave ? s_w[w] : 0u;
  return offsets[blockIdx.x] + wave_off + (unsigned int)__popcll(bal & ((1ull << lane) - 1ull));
}

}  // namespace ndt
