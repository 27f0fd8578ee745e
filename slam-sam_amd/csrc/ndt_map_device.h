// ndt_map_device.h -- what the voxel map's kernels share across translation units (ndt_map.hip, ndt_map_state.hip,
// ndt_map_carve.hip): the table's constants, the words of VoxelMap::stats / tsel, the hash, the probe that claims a slot
// and the one that only looks, the box predicate of a selection and the wave reductions.  Device code only; include it
// after hip_runtime.
#pragma once

namespace ndt {

constexpr int MAP_THREADS = 256, MAP_WAVES = MAP_THREADS / 64;
constexpr int MAP_XROUNDS = 4;                         // slots per thread of the export's compaction
constexpr int MAP_XTILE = MAP_THREADS * MAP_XROUNDS;
constexpr unsigned long long MAP_EMPTY = ~0ull;
constexpr int MAP_BIAS = 1 << 20;                      // |ijk| < 2^20 per axis: 21 bits each once biased
constexpr float MAP_LIMIT = 1048576.0f;
// words of VoxelMap::stats
enum { MS_FINITE = 0, MS_OOR = 1, MS_MIN = 2, MS_MAX = 5, MS_PROBE_FAIL = 8, MS_WORDS = 16 };
// words of VoxelMap::tsel: ijk box, number and point total (64 bits) of the occupied voxels a selection's box holds,
// and the leaves its finalize launch accepted
enum { TS_MIN = 0, TS_MAX = 3, TS_VOXELS = 6, TS_POINTS = 8, TS_VALID = 10, TS_WORDS = 16 };

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
  const int vi = (int)(key & 0x1fffffull) - MAP_BIAS, vj = (int)((key >> 21) & 0x1fffffull) - MAP_BIAS,
            vk = (int)(key >> 42) - MAP_BIAS;
  return vi >= sel.lo[0] && vi <= sel.hi[0] && vj >= sel.lo[1] && vj <= sel.hi[1] && vk >= sel.lo[2] && vk <= sel.hi[2];
}

}  // namespace ndt
