// ndt_map_device.h -- what the voxel map's kernels share across translation units (ndt_map.hip, ndt_map_state.hip,
// ndt_map_carve.hip, ndt_map_repose.hip; ndt_target.hip for the key alone): the table's constants, the words of VoxelMap::stats / tsel, the
// 63-bit key and its inverse (map_key / map_ijk: the only place that knows the layout), the hash, the probe that claims
// a slot and the one that only looks, the box predicate of a selection, the wave reductions, the block's reduction of an
// ijk box (map_box_waves / map_box_commit around the kernel's barrier), the statistics of a batch of records
// (map_record_stats) and one slot's move into a fresh table
// (map_move_slot: what growth, crop and carve do with a voxel that stays).  Device code only.
#pragma once

#include "ndt_engine.h"   // MapTable

namespace ndt {

constexpr int MAP_THREADS = 256, MAP_WAVES = MAP_THREADS / 64;
constexpr int MAP_XROUNDS = 4;                         // slots per thread of the export's compaction
constexpr int MAP_XTILE = MAP_THREADS * MAP_XROUNDS;
constexpr unsigned long long MAP_EMPTY = ~0ull;
constexpr int MAP_BIAS = 1 << 20;                      // |ijk| < 2^20 per axis: 21 bits each once biased
constexpr float MAP_LIMIT = 1048576.0f;
// words of VoxelMap::stats
enum { MS_FINITE = 0, MS_OOR = 1, MS_MIN = 2, MS_MAX = 5, MS_PROBE_FAIL = 8, MS_WORDS = 16 };
// ... and those a batch of voxel RECORDS adds (the state import's key pass, the re-pose's record pass)
enum { MS_BAD_COUNT = 9, MS_POINTS = 10 /* 64 bits */ };
// words of VoxelMap::tsel: ijk box, number and point total (64 bits) of the occupied voxels a selection's box holds,
// and the leaves its finalize launch accepted
enum { TS_MIN = 0, TS_MAX = 3, TS_VOXELS = 6, TS_POINTS = 8, TS_VALID = 10, TS_WORDS = 16 };

// The voxel key: (k, j, i) biased into 21 bits each -- 63 bits that order as PCL's dense index does; |ijk| < 2^20.
__device__ __forceinline__ unsigned long long map_key(int i, int j, int k) {
  return ((unsigned long long)(k + MAP_BIAS) << 42) | ((unsigned long long)(j + MAP_BIAS) << 21) |
         (unsigned long long)(i + MAP_BIAS);
}
__device__ __forceinline__ void map_ijk(unsigned long long key, int (&v)[3]) {
  v[0] = (int)(key & 0x1fffffull) - MAP_BIAS;
  v[1] = (int)((key >> 21) & 0x1fffffull) - MAP_BIAS;
  v[2] = (int)(key >> 42) - MAP_BIAS;
}

__device__ __forceinline__ unsigned long long map_hash(unsigned long long k) {  // splitmix64's finaliser
  k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27; k *= 0x94d049bb133111ebull;
  k ^= k >> 31;
  return k;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}

// The slot of `key` in the table (linear probing from its hash): the position whose key word holds it, claimed with
// atomicCAS if no position does yet.  *claimed: this call put the key there.  -1 if all `mask + 1` positions hold other
// keys (cannot happen at a load of 1/2).  A plain load may show a stale EMPTY, never a wrong key (key words are written
// once): the CAS then tells the truth.
__device__ __forceinline__ long long map_slot_of(unsigned long long* __restrict__ tkeys, unsigned long long mask,
                                                 unsigned long long key, bool* claimed) {
  unsigned long long s = map_hash(key) & mask;
  *claimed = false;
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    unsigned long long cur = tkeys[s];
    if (cur == MAP_EMPTY) {
      cur = atomicCAS(tkeys + s, MAP_EMPTY, key);
      if (cur == MAP_EMPTY) { *claimed = true; return (long long)s; }
    }
    if (cur == key) return (long long)s;
    s = (s + 1) & mask;
  }
  return -1;
}

// The slot that holds `key`, or -1 if the table does not hold it: the same probe sequence, read only, ended by the first
// empty position (nothing is ever deleted in place) or after all `mask + 1` positions.  For a table no launch in flight
// inserts into.
__device__ __forceinline__ long long map_find(const unsigned long long* __restrict__ tkeys, unsigned long long mask,
                                              unsigned long long key) {
  unsigned long long s = map_hash(key) & mask;
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    const unsigned long long cur = tkeys[s];
    if (cur == key) return (long long)s;
    if (cur == MAP_EMPTY) return -1;
    s = (s + 1) & mask;
  }
  return -1;
}

// What a selection takes: the occupied slots with count >= min_points and, in the BOX instantiations, a voxel inside
// lo <= ijk <= hi (absolute voxel coordinates, both ends included).
struct MapSel {
  int min_points;
  int lo[3], hi[3];
};

__device__ __forceinline__ bool map_in_box(unsigned long long key, const MapSel& sel) {
  int v[3];
  map_ijk(key, v);
  return v[0] >= sel.lo[0] && v[0] <= sel.hi[0] && v[1] >= sel.lo[1] && v[1] <= sel.hi[1] && v[2] >= sel.lo[2] && v[2] <= sel.hi[2];
}

// The ijk box of what a block's threads hold (mn / mx; a thread without a voxel brings INT_MAX / INT_MIN), reduced into
// the words bmin[0..2] / bmax[0..2] with at most one integer atomic per word and block.  Split around the barrier, which
// the kernel owns (it may reduce its counters across the same one), as ndt_compact_device.h's helpers are; `box` is the
// kernel's own __shared__ array.
// in front of the barrier: the wave's box to box[wave]
__device__ __forceinline__ void map_box_waves(const int (&mn)[3], const int (&mx)[3], int (&box)[MAP_WAVES][6]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int lo = wave_min(mn[a]), hi = wave_max(mx[a]);
    if ((threadIdx.x & 63u) == 0) { box[threadIdx.x >> 6][a] = lo; box[threadIdx.x >> 6][3 + a] = hi; }
  }
}
// behind it: threads 0..5 fold the waves, one word each; a block without a voxel writes nothing
__device__ __forceinline__ void map_box_commit(const int (&box)[MAP_WAVES][6], int* __restrict__ bmin, int* __restrict__ bmax) {
  if (threadIdx.x < 6) {
    const int t = (int)threadIdx.x;
    int v = box[0][t];
#pragma unroll
    for (int w = 1; w < MAP_WAVES; ++w) v = t < 3 ? min(v, box[w][t]) : max(v, box[w][t]);
    if (t < 3) { if (v != INT_MAX) atomicMin(bmin + t, v); }
    else if (v != INT_MIN) atomicMax(bmax + (t - 3), v);
  }
}

// The statistics of a batch of voxel records, as the host reads them under the import's one wait: how many records are
// out of the coordinate range (oor) and how many have count < 1 (bad), the ijk box (mn / mx) and the 64-bit point total
// (pts) of the valid ones -- every thread of the block brings its record's (a thread without one: 0, 0, 0 and the empty
// box); one integer atomic per word and block.  Holds the block's barrier: every thread calls it, once.
__device__ __forceinline__ void map_record_stats(int oor, int bad, unsigned long long pts, const int (&mn)[3], const int (&mx)[3],
                                                 int* __restrict__ stats) {
  __shared__ int red[MAP_WAVES][2], box[MAP_WAVES][6];
  __shared__ unsigned long long red_pts[MAP_WAVES];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  oor = wave_sum(oor);
  bad = wave_sum(bad);
  pts = wave_sum_u64(pts);
  if (lane == 0) { red[wave][0] = oor; red[wave][1] = bad; red_pts[wave] = pts; }
  map_box_waves(mn, mx, box);
  __syncthreads();
  map_box_commit(box, stats + MS_MIN, stats + MS_MAX);
  if (threadIdx.x == 6 || threadIdx.x == 7) {
    const int t = (int)threadIdx.x - 6;
    int v = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) v += red[w][t];
    if (v) atomicAdd(stats + (t == 0 ? MS_OOR : MS_BAD_COUNT), v);
  } else if (threadIdx.x == 8) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) v += red_pts[w];
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(stats + MS_POINTS), v);
  }
}

// The occupied slot i of table `o` (its key: `key`) moves to the fresh table `t` with its sums, its count and -- where
// the tables have them -- its nine moments as they are.  false: the probe found no position (counted in stats; cannot
// happen at a load of 1/2), nothing was written.
__device__ __forceinline__ bool map_move_slot(const engine::MapTable& o, long long i, unsigned long long key,
                                              const engine::MapTable& t, int* __restrict__ stats) {
  bool claimed;
  const long long s = map_slot_of(t.keys, (unsigned long long)(t.capacity - 1), key, &claimed);
  if (s < 0) { atomicAdd(stats + MS_PROBE_FAIL, 1); return false; }
  // (every load in front of the first store: the pointers of a struct carry no __restrict__, and a store in between
  // would make the loads behind it wait for it)
  const float4 sm = o.sums[i];
  const int c = o.cnt[i];
  double q[9];
  if (t.mom) {
#pragma unroll
    for (int a = 0; a < 9; ++a) q[a] = o.mom[(size_t)i * 9 + a];
  }
  t.sums[s] = sm;
  t.cnt[s] = c;
  if (t.mom) {
#pragma unroll
    for (int a = 0; a < 9; ++a) t.mom[(size_t)s * 9 + a] = q[a];
  }
  return true;
}

}  // namespace ndt
