// ndt_map.hip -- the sparse voxel map accumulated scan by scan (ndt_map_*, see ndt_engine.h: VoxelMap).
// pcl::VoxelGrid centroids of EVERYTHING added so far, without keeping the points and without a dense index
// (ref: run/pipeline_ins_map_distribution.cpp:281-377 keeps every scan until shutdown and filters the concatenation once).
//   add      [transform] -> keys + range check (ONE host wait: refusal / growth are decided before anything is written)
//            -> insert (atomicCAS on the key word; the table position is the slot) -> the build's stable radix sort of
//            (slot, point index) and its run search -> one thread per run continues the voxel's float sums in input order
//   export   compaction of the slots that pass min_points (k_map_xcount / k_map_xemit: four-round tiles of ballots; the
//            block offsets by the engine's one scan, launch_filter_scan) -> sort by the voxel key relative to the map's
//            bounding box (one 32-bit sort, or two: low word then high word) -> centroids
// Integer atomics only (the CAS, the block totals of the statistics); no kernel waits for another block, every probe loop
// is bounded by the capacity.  Which slot a voxel gets depends on the race, on the hash and on the capacity -- what the
// slot holds does not: a voxel's sums are ((old + p1) + p2) ... over its points in input order, and the export orders by key.
//   moments  (ndt_map_enable_moments) the same add also continues, per voxel, the nine f64 sums the target build reduces a
//            voxel's points to; ndt_set_target_from_map_moments selects the voxels of a box with the export's count / scan /
//            compaction / key sort under a predicate (ONE host wait: selection count, ijk box and point total decide the
//            refusals and size the grid) and hands each to the ordinary build's finalize_leaf (launch_map_finalize).
// Crop, state export and state import are in ndt_map_state.hip, the carve in ndt_map_carve.hip, the re-pose in
// ndt_map_repose.hip; the constants and device helpers these files use (key, probes, box reduction, a slot's move) are in ndt_map_device.h, and the host functions
// of this file that the others call -- map_replace_table, the one way a table is replaced, among them -- are declared in
// ndt_engine.h.
#include "ndt_engine.h"
#include "ndt_map_device.h"

namespace ndt {

namespace {

__device__ __forceinline__ bool map_finite3(float a, float b, float c) {
  return isfinite(a) && isfinite(b) && isfinite(c);
}

// Voxel key per point: floor(p * inv_leaf) per axis in f32 (the downsample's arithmetic), (k, j, i) biased into 21 bits
// each -- a 63-bit key that orders as PCL's dense index does.  MAP_EMPTY for a non-finite point (skipped, counted) and
// for a finite one outside the coordinate range (counted: the host refuses the whole add).  The batch's statistics go
// to `stats` with one integer atomic per word and block.
__global__ void __launch_bounds__(MAP_THREADS) k_map_keys(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ z, int n, float inv_leaf,
                                                         unsigned long long* __restrict__ pkey, int* __restrict__ stats) {
  __shared__ int red[MAP_WAVES][2], box[MAP_WAVES][6];
  const int i = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  int fin = 0, oor = 0;
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  if (i < n) {
    const float a = x[i], b = y[i], c = z[i];
    unsigned long long key = MAP_EMPTY;
    if (map_finite3(a, b, c)) {
      fin = 1;
      const float fi = floorf(a * inv_leaf), fj = floorf(b * inv_leaf), fk = floorf(c * inv_leaf);
      if (fabsf(fi) < MAP_LIMIT && fabsf(fj) < MAP_LIMIT && fabsf(fk) < MAP_LIMIT) {
        const int vi = (int)fi, vj = (int)fj, vk = (int)fk;
        mn[0] = mx[0] = vi; mn[1] = mx[1] = vj; mn[2] = mx[2] = vk;
        key = map_key(vi, vj, vk);
      } else {
        oor = 1;
      }
    }
    pkey[i] = key;
  }
  fin = wave_sum(fin);
  oor = wave_sum(oor);
  if ((threadIdx.x & 63u) == 0) { red[threadIdx.x >> 6][0] = fin; red[threadIdx.x >> 6][1] = oor; }
  map_box_waves(mn, mx, box);
  __syncthreads();
  map_box_commit(box, stats + MS_MIN, stats + MS_MAX);
  if (threadIdx.x == 6 || threadIdx.x == 7) {   // (the two counters: the threads of that wave the box leaves idle)
    const int t = (int)threadIdx.x - 6;          // MS_FINITE, MS_OOR
    int v = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) v += red[w][t];
    if (v) atomicAdd(stats + t, v);
  }
}

// slot per point (the sort key of the grouping; `mask + 1`, the sentinel, for a skipped point) + the number of
// voxels this batch created, added to *nvox
__global__ void __launch_bounds__(MAP_THREADS) k_map_insert(const unsigned long long* __restrict__ pkey, int n,
                                                           unsigned long long* __restrict__ tkeys, unsigned long long mask,
                                                           uint32_t* __restrict__ slots, unsigned long long* __restrict__ nvox,
                                                           int* __restrict__ stats) {
  __shared__ int red[MAP_WAVES];
  const int i = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  int fresh = 0;
  if (i < n) {
    const unsigned long long key = pkey[i];
    uint32_t slot = (uint32_t)(mask + 1);
    if (key != MAP_EMPTY) {
      bool claimed;
      const long long s = map_slot_of(tkeys, mask, key, &claimed);
      if (s >= 0) slot = (uint32_t)s;
      else atomicAdd(stats + MS_PROBE_FAIL, 1);
      fresh = claimed ? 1 : 0;
    }
    slots[i] = slot;
  }
  fresh = wave_sum(fresh);
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = fresh;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) c += red[w];
    if (c) atomicAdd(nvox, (unsigned long long)c);
  }
}

// Run r of the slot-sorted batch = points vals_sorted[start .. start + cnt) of one voxel, in input order (the radix sort
// is stable): its sums go on from what the map holds, one point at a time, as k_voxel_centroids adds them from zero.
// MOM: so do its nine f64 moment sums -- a, b, c hold f32 values, so every product is exact in f64 and ss += a * b rounds
// once whether or not it is contracted; the chains run in input order like the oracle's.
template <bool MOM>
__global__ void __launch_bounds__(MAP_THREADS) k_map_accumulate(const int* __restrict__ d_nleaf, const int* __restrict__ leaf_start,
                                                               const int* __restrict__ leaf_cnt,
                                                               const uint32_t* __restrict__ keys_sorted,
                                                               const uint32_t* __restrict__ vals_sorted,
                                                               const float* __restrict__ px, const float* __restrict__ py,
                                                               const float* __restrict__ pz, const float* __restrict__ pi,
                                                               float4* __restrict__ sums, int* __restrict__ cnt,
                                                               double* __restrict__ mom) {
  const int r = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  if (r >= d_nleaf[0]) return;
  const int start = leaf_start[r], c = leaf_cnt[r];
  const uint32_t slot = keys_sorted[start];
  float4 s = sums[slot];
  double q[9];
  if (MOM) {
#pragma unroll
    for (int a = 0; a < 9; ++a) q[a] = mom[(size_t)slot * 9 + a];
  }
  for (int j = 0; j < c; ++j) {
    const uint32_t p = vals_sorted[start + j];
    const float fx = px[p], fy = py[p], fz = pz[p];
    s.x += fx; s.y += fy; s.z += fz;
    if (pi) s.w += pi[p];
    if (MOM) {
      const double a = (double)fx, b = (double)fy, d = (double)fz;
      q[0] += a; q[1] += b; q[2] += d;
      q[3] += a * a; q[4] += a * b; q[5] += a * d;
      q[6] += b * b; q[7] += b * d; q[8] += d * d;
    }
  }
  sums[slot] = s;
  cnt[slot] += c;
  if (MOM) {
#pragma unroll
    for (int a = 0; a < 9; ++a) mom[(size_t)slot * 9 + a] = q[a];
  }
}

// growth: every occupied slot of the old table moves to the new one with its sums and its count as they are
__global__ void __launch_bounds__(MAP_THREADS) k_map_rehash(MapTable o, MapTable t, int* __restrict__ stats) {
  const long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
  if (i >= o.capacity) return;
  const unsigned long long key = o.keys[i];
  if (key != MAP_EMPTY) map_move_slot(o, i, key, t, stats);
}

// ---- export ----
template <bool BOX>
__device__ __forceinline__ bool map_pass(const unsigned long long* __restrict__ tkeys, const int* __restrict__ cnt,
                                         long long slot, long long cap, const MapSel& sel) {
  if (slot >= cap) return false;
  const unsigned long long key = tkeys[slot];
  if (key == MAP_EMPTY) return false;
  if (BOX && !map_in_box(key, sel)) return false;
  return cnt[slot] >= sel.min_points;
}

// BOX: the same pass reduces, over the OCCUPIED voxels inside the box whatever their count, the ijk box, their number
// and their point total into tsel (TS_* words; one integer atomic per word and block, as k_map_keys)
template <bool BOX>
__global__ void __launch_bounds__(MAP_THREADS) k_map_xcount(const unsigned long long* __restrict__ tkeys,
                                                           const int* __restrict__ cnt, long long cap, MapSel sel,
                                                           unsigned int* __restrict__ counts, int* __restrict__ tsel) {
  __shared__ unsigned int s_w[MAP_WAVES];
  __shared__ int box[MAP_WAVES][6], red_vox[MAP_WAVES];
  __shared__ unsigned long long red_pts[MAP_WAVES];
  unsigned int c = 0;
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN}, nvox = 0;
  unsigned long long pts = 0;
#pragma unroll
  for (int r = 0; r < MAP_XROUNDS; ++r) {
    const long long slot = (long long)blockIdx.x * MAP_XTILE + r * MAP_THREADS + threadIdx.x;
    if (BOX) {
      bool pass = false;
      if (slot < cap) {
        const unsigned long long key = tkeys[slot];
        if (key != MAP_EMPTY && map_in_box(key, sel)) {
          const int n = cnt[slot];
          int v[3];
          map_ijk(key, v);
#pragma unroll
          for (int a = 0; a < 3; ++a) { mn[a] = min(mn[a], v[a]); mx[a] = max(mx[a], v[a]); }
          ++nvox;
          pts += (unsigned long long)n;
          pass = n >= sel.min_points;
        }
      }
      c += (unsigned int)__popcll(__ballot(pass));
    } else {
      c += (unsigned int)__popcll(__ballot(map_pass<false>(tkeys, cnt, slot, cap, sel)));
    }
  }
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  if (BOX) {
    nvox = wave_sum(nvox);
    pts = wave_sum_u64(pts);
    if (lane == 0) { red_vox[wave] = nvox; red_pts[wave] = pts; }
    map_box_waves(mn, mx, box);
  }
  if (lane == 0) s_w[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int t = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) t += s_w[w];
    counts[blockIdx.x] = t;
  }
  if (BOX) {
    map_box_commit(box, tsel + TS_MIN, tsel + TS_MAX);
    if (threadIdx.x == 6) {
      int v = 0;
#pragma unroll
      for (int w = 0; w < MAP_WAVES; ++w) v += red_vox[w];
      if (v) atomicAdd(tsel + TS_VOXELS, v);
    } else if (threadIdx.x == 7) {
      unsigned long long v = 0;
#pragma unroll
      for (int w = 0; w < MAP_WAVES; ++w) v += red_pts[w];
      if (v) atomicAdd(reinterpret_cast<unsigned long long*>(tsel + TS_POINTS), v);
    }
  }
}

// the key relative to the map's bounding box: (k - min_k, j - min_j, i - min_i) packed into bz + by + bx bits
struct MapKeyBox {
  int mn[3];
  int bx, by;
};

// the selected slots, compacted (in table order: the sort that follows puts them in key order), and their relative keys
template <bool BOX>
__global__ void __launch_bounds__(MAP_THREADS) k_map_xemit(const unsigned long long* __restrict__ tkeys,
                                                          const int* __restrict__ cnt, long long cap, MapSel sel,
                                                          const unsigned int* __restrict__ offsets, MapKeyBox box,
                                                          uint32_t* __restrict__ xslot, uint32_t* __restrict__ klo,
                                                          uint32_t* __restrict__ khi) {
  __shared__ unsigned int s_w[MAP_XROUNDS][MAP_WAVES];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  bool keep[MAP_XROUNDS];
  unsigned long long bal[MAP_XROUNDS];
#pragma unroll
  for (int r = 0; r < MAP_XROUNDS; ++r) {
    const long long slot = (long long)blockIdx.x * MAP_XTILE + r * MAP_THREADS + threadIdx.x;
    keep[r] = map_pass<BOX>(tkeys, cnt, slot, cap, sel);
    bal[r] = __ballot(keep[r]);
    if (lane == 0) s_w[r][wave] = (unsigned int)__popcll(bal[r]);
  }
  __syncthreads();
  unsigned int before = offsets[blockIdx.x];
#pragma unroll
  for (int r = 0; r < MAP_XROUNDS; ++r) {
    unsigned int wave_off = 0, round_total = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) {
      const unsigned int t = s_w[r][w];
      wave_off += w < wave ? t : 0u;
      round_total += t;
    }
    if (keep[r]) {
      const long long slot = (long long)blockIdx.x * MAP_XTILE + r * MAP_THREADS + threadIdx.x;
      const unsigned int pos = before + wave_off + (unsigned int)__popcll(bal[r] & ((1ull << lane) - 1ull));
      int v[3];
      map_ijk(tkeys[slot], v);   // (inside the box: no difference is negative)
      const unsigned long long vi = (unsigned long long)(v[0] - box.mn[0]), vj = (unsigned long long)(v[1] - box.mn[1]),
                               vk = (unsigned long long)(v[2] - box.mn[2]);
      const unsigned long long rk = (vk << (box.bx + box.by)) | (vj << box.bx) | vi;
      xslot[pos] = (uint32_t)slot;
      klo[pos] = (uint32_t)rk;
      if (khi) khi[pos] = (uint32_t)(rk >> 32);
    }
    before += round_total;
  }
}

// between the two sorts: the high words and the slots in low-word order
__global__ void __launch_bounds__(MAP_THREADS) k_map_xgather(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ khi,
                                                            const uint32_t* __restrict__ xslot, int m,
                                                            uint32_t* __restrict__ khi2, uint32_t* __restrict__ xslot2) {
  const int i = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  if (i >= m) return;
  const uint32_t p = perm[i];
  khi2[i] = khi[p];
  xslot2[i] = xslot[p];
}

// output point r = the voxel slots[order[r]]: every field sum / (float)count, as k_voxel_centroids divides
__global__ void __launch_bounds__(MAP_THREADS) k_map_xcentroids(const uint32_t* __restrict__ order, const uint32_t* __restrict__ slots,
                                                               int m, const float4* __restrict__ sums, const int* __restrict__ cnt,
                                                               float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz,
                                                               float* __restrict__ oi, int32_t* __restrict__ ocount) {
  const int r = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  if (r >= m) return;
  const uint32_t slot = slots[order[r]];
  const float4 s = sums[slot];
  const int c = cnt[slot];
  const float nf = (float)c;
  ox[r] = s.x / nf; oy[r] = s.y / nf; oz[r] = s.z / nf;
  if (oi) oi[r] = s.w / nf;
  if (ocount) ocount[r] = c;
}

}  // namespace

namespace engine {
namespace {

constexpr int64_t MAP_DEFAULT_CAPACITY = 1ll << 18;

}  // namespace

// ---- the host side ndt_map_state.hip shares (declared in ndt_engine.h) ----

void map_free_table(MapTable& t) {
  if (t.keys) (void)hipFree(t.keys);
  if (t.sums) (void)hipFree(t.sums);
  if (t.cnt) (void)hipFree(t.cnt);
  if (t.mom) (void)hipFree(t.mom);
  t = MapTable{};
}

// an empty table of `cap` slots (keys ~0, sums, counts and -- with_moments -- moments zero), written on the engine's stream
int map_alloc_table(ndt_handle* h, int64_t cap, bool with_moments, MapTable* t) {
  *t = MapTable{};
  const size_t n = (size_t)cap;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&t->keys), n * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->sums), n * sizeof(float4));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->cnt), n * sizeof(int));
  if (e == hipSuccess && with_moments) e = hipMalloc(reinterpret_cast<void**>(&t->mom), n * 9 * sizeof(double));
  if (e == hipSuccess) e = hipMemsetAsync(t->keys, 0xFF, n * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->sums, 0, n * sizeof(float4), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->cnt, 0, n * sizeof(int), h->stream);
  if (e == hipSuccess && with_moments) e = hipMemsetAsync(t->mom, 0, n * 9 * sizeof(double), h->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    map_free_table(*t);
    return fail(h, e == hipErrorOutOfMemory ? NDT_ERR_ALLOC : NDT_ERR_HIP, std::string("voxel map table: ") + hipGetErrorString(e));
  }
  t->capacity = cap;
  return NDT_OK;
}

int64_t map_pow2_at_least(int64_t v) {
  int64_t c = 64;
  while (c < v) c <<= 1;
  return c;
}

// n_voxels as the device counts it (the insert launches before this point have run when the call returns)
int map_refresh_voxel_count(ndt_handle* h, VoxelMap& m) {
  if (!m.nvox_stale) return NDT_OK;
  HIP_TRY(h, hipMemcpyAsync(m.nvox_h.h, m.nvox.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  m.n_voxels = (int64_t)m.nvox_h.h[0];
  m.nvox_stale = false;
  return NDT_OK;
}

int map_replace_table(ndt_handle* h, VoxelMap& m, int64_t new_cap, const char* what,
                      const std::function<int(const MapTable&)>& launch, int64_t kept) {
  hipStream_t s = h->stream;
  const bool counted = kept == MAP_KEPT_COUNTED;   // the launch counts the voxels it creates in nvox[1]
  const bool selective = kept >= 0;
  MapTable fresh;
  int rc = map_alloc_table(h, new_cap, m.moments, &fresh);
  if (rc) return rc;   // the map is as it was
  hipError_t e = hipSuccess;
  if (selective) e = hipMemcpyAsync(m.tsel.p, m.tsel_h.h + TS_WORDS, TS_WORDS * sizeof(int), hipMemcpyHostToDevice, s);
  if (counted) e = hipMemsetAsync(m.nvox.p + 1, 0, sizeof(unsigned long long), s);
  if (e == hipSuccess) {
    rc = launch(fresh);
    if (rc) {   // (the launch has reported it; what it enqueued may still write to the fresh table)
      (void)hipStreamSynchronize(s);
      (void)hipGetLastError();
      map_free_table(fresh);
      return rc;
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess && selective) e = hipMemcpyAsync(m.tsel_h.h, m.tsel.p, TS_WORDS * sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && counted) e = hipMemcpyAsync(m.nvox_h.h + 1, m.nvox.p + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // (a replacement is rare: the old table is freed behind its last reader)
  if (e == hipSuccess && counted) kept = (int64_t)m.nvox_h.h[1];
  if (e == hipSuccess && (selective || counted)) {   // the next add reads the device's counter
    m.nvox_h.h[0] = (unsigned long long)kept;
    e = hipMemcpy(m.nvox.p, m.nvox_h.h, sizeof(unsigned long long), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    map_free_table(fresh);
    return fail(h, NDT_ERR_HIP, std::string(what) + hipGetErrorString(e));
  }
  map_free_table(m.tab);
  m.tab = fresh;
  ++m.change;
  if (selective || counted) {
    m.n_voxels = kept;
    m.nvox_stale = false;
    if (selective && kept > 0)
      for (int a = 0; a < 3; ++a) { m.mn[a] = m.tsel_h.h[TS_MIN + a]; m.mx[a] = m.tsel_h.h[TS_MAX + a]; }
  }
  return NDT_OK;
}

// Growth (refill == nullptr): every voxel moves as it is into a table of new_cap slots, and n_grows counts it.  With a
// refill the fresh table is filled by the caller's own launches instead, which count the voxels they create (the re-pose
// of ndt_map_repose.hip: the voxels do not move as they are); that is no growth, and the ijk box is the caller's to set.
int map_grow_table(ndt_handle* h, VoxelMap& m, int64_t new_cap, const MapRefill* refill) {
  const std::function<int(const MapTable&)> rehash = [&](const MapTable& fresh) {
    hipLaunchKernelGGL(k_map_rehash, dim3((unsigned)((m.tab.capacity + MAP_THREADS - 1) / MAP_THREADS)), dim3(MAP_THREADS), 0,
                       h->stream, m.tab, fresh, m.stats.p);
    return (int)NDT_OK;
  };
  const int rc = map_replace_table(h, m, new_cap, refill ? refill->what : "voxel map growth: ", refill ? refill->launch : rehash,
                                   refill ? MAP_KEPT_COUNTED : -1);
  if (rc == NDT_OK && !refill) ++m.n_grows;
  return rc;
}

// The batch's n keys (m.pkey; MAP_EMPTY: skipped) get their slots in table `t` (k_map_insert: *d_nvox -- for the map's own
// table the device's voxel counter -- goes up by the voxels created), then the stable sort of (slot, index) and the run search: run r of *keys_sorted / *vals_sorted is one
// voxel's entries in input order (h->nleaf, h->leaf_start, h->leaf_cnt).  After group_scratch(n, n + 1); enqueued, not awaited.
int map_group_batch(ndt_handle* h, VoxelMap& m, size_t n, const MapTable& t, unsigned long long* d_nvox,
                    const uint32_t** keys_sorted, const uint32_t** vals_sorted) {
  hipStream_t s = h->stream;
  const unsigned blocks = (unsigned)((n + MAP_THREADS - 1) / MAP_THREADS);
  hipLaunchKernelGGL(k_map_insert, dim3(blocks), dim3(MAP_THREADS), 0, s, m.pkey.p, (int)n, t.keys,
                     (unsigned long long)(t.capacity - 1), h->sort.keys.p, d_nvox, m.stats.p);
  int passes = 0;
  int rc = sort_put_plan(h, h->gd.p, sort_key_bits(t.capacity), (int)t.capacity, &passes);   // (the sentinel `capacity` sorts behind every slot)
  if (rc) return rc;
  SortedPairs sorted;
  HIP_TRY(h, sort_keyed(h->sort, n, h->gd.p, passes, SORT_COUNT_FIRST, s, &sorted));
  *keys_sorted = sorted.keys;
  *vals_sorted = sorted.vals;
  HIP_TRY(h, find_runs(h, sorted.keys, n, /*min_pts=*/1, /*fused=*/false));
  return NDT_OK;
}

namespace {

// One batch in device memory (di may be null in a map without intensity) under an optional pose.
int map_add_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, const float* di, size_t n,
                   const double* pose16) {
  VoxelMap& m = *h->map;
  if (n == 0) return NDT_OK;
  if (n > (size_t)std::numeric_limits<int>::max() / 2) return fail(h, NDT_ERR_INVALID_ARG, "cloud too large");
  settle_discard_keep_grid(h);
  hipStream_t s = h->stream;
  // every allocation of the add except the table's growth, before anything is written
  HIP_TRY(h, m.pkey.ensure(n));
  if (pose16) {
    HIP_TRY(h, m.px.ensure(n));
    HIP_TRY(h, m.py.ensure(n));
    HIP_TRY(h, m.pz.ensure(n));
  }
  int rc = group_scratch(h, n, n + 1);
  if (rc) return rc;
  const float *qx = dx, *qy = dy, *qz = dz;
  if (pose16) {
    launch_transform_append(dx, dy, dz, n, pose16, m.px.p, m.py.p, m.pz.p, s);
    qx = m.px.p; qy = m.py.p; qz = m.pz.p;
  }
  const unsigned blocks = (unsigned)((n + MAP_THREADS - 1) / MAP_THREADS);
  HIP_TRY(h, hipMemcpyAsync(m.stats.p, m.stats_h.h + MS_WORDS, MS_WORDS * sizeof(int), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_map_keys, dim3(blocks), dim3(MAP_THREADS), 0, s, qx, qy, qz, (int)n, m.inv_leaf, m.pkey.p, m.stats.p);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(m.stats_h.h, m.stats.p, MS_WORDS * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(m.nvox_h.h, m.nvox.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));   // the add's one host wait: range check and growth decision
  m.n_voxels = (int64_t)m.nvox_h.h[0];
  m.nvox_stale = false;
  const int* st = m.stats_h.h;
  if (st[MS_OOR] > 0)
    return fail(h, NDT_ERR_GRID_OVERFLOW, std::to_string(st[MS_OOR]) + " point(s) beyond the map's coordinate range (|voxel index| < 2^20 per axis); nothing was added");
  const int64_t n_finite = st[MS_FINITE];
  const int64_t want = map_pow2_at_least(2 * (m.n_voxels + (int64_t)n));
  if (want > m.tab.capacity) {
    if (want > MAP_MAX_CAPACITY) return fail(h, NDT_ERR_ALLOC, "voxel map: more than 2^30 table slots needed");
    rc = map_grow_table(h, m, want);
    if (rc) return rc;
  }
  // from here on the map changes
  ++m.change;
  ++m.n_adds;
  m.n_dropped += (int64_t)n - n_finite;
  if (n_finite == 0) return NDT_OK;
  for (int a = 0; a < 3; ++a) {
    m.mn[a] = m.n_points ? std::min(m.mn[a], st[MS_MIN + a]) : st[MS_MIN + a];
    m.mx[a] = m.n_points ? std::max(m.mx[a], st[MS_MAX + a]) : st[MS_MAX + a];
  }
  m.n_points += n_finite;
  m.nvox_stale = true;
  const uint32_t *keys_sorted = nullptr, *vals_sorted = nullptr;
  rc = map_group_batch(h, m, n, m.tab, m.nvox.p, &keys_sorted, &vals_sorted);
  if (rc) return rc;
  if (m.moments)
    hipLaunchKernelGGL(k_map_accumulate<true>, dim3(blocks), dim3(MAP_THREADS), 0, s, h->nleaf.p, h->leaf_start.p, h->leaf_cnt.p,
                       keys_sorted, vals_sorted, qx, qy, qz, m.with_intensity ? di : nullptr,
                       m.tab.sums, m.tab.cnt, m.tab.mom);
  else
    hipLaunchKernelGGL(k_map_accumulate<false>, dim3(blocks), dim3(MAP_THREADS), 0, s, h->nleaf.p, h->leaf_start.p, h->leaf_cnt.p,
                       keys_sorted, vals_sorted, qx, qy, qz, m.with_intensity ? di : nullptr,
                       m.tab.sums, m.tab.cnt, static_cast<double*>(nullptr));
  HIP_TRY(h, hipGetLastError());
  // the caller's arrays (and the engine's scratch) are free again when the call returns
  HIP_TRY(h, hipStreamSynchronize(s));
  return NDT_OK;
}

MapSel sel_all(int min_points) {
  MapSel sel{};
  sel.min_points = min_points;
  return sel;
}

}  // namespace

// the voxels a selection takes (count + scan, awaited); the block offsets stay in xcounts.  box: the selection is
// limited to sel.lo .. sel.hi, and tsel_h receives the TS_* words of the occupied voxels inside (same wait)
int map_export_count(ndt_handle* h, VoxelMap& m, const MapSel& sel, bool box, size_t* total) {
  *total = 0;
  int rc = map_refresh_voxel_count(h, m);
  if (rc) return rc;
  if (m.n_voxels == 0) return NDT_OK;
  hipStream_t s = h->stream;
  const int nb = (int)((m.tab.capacity + MAP_XTILE - 1) / MAP_XTILE);
  HIP_TRY(h, m.xcounts.ensure((size_t)nb + 2));
  if (box) {
    HIP_TRY(h, hipMemcpyAsync(m.tsel.p, m.tsel_h.h + TS_WORDS, TS_WORDS * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_map_xcount<true>, dim3((unsigned)nb), dim3(MAP_THREADS), 0, s, m.tab.keys, m.tab.cnt, (long long)m.tab.capacity, sel,
                       m.xcounts.p, m.tsel.p);
  } else {
    hipLaunchKernelGGL(k_map_xcount<false>, dim3((unsigned)nb), dim3(MAP_THREADS), 0, s, m.tab.keys, m.tab.cnt, (long long)m.tab.capacity, sel,
                       m.xcounts.p, static_cast<int*>(nullptr));
  }
  launch_filter_scan(m.xcounts.p, nb, m.xcounts.p + nb + 1, s);   // (xcounts[nb] receives the sum as well: read below)
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(m.nvox_h.h + 1, m.xcounts.p + nb, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
  if (box) HIP_TRY(h, hipMemcpyAsync(m.tsel_h.h, m.tsel.p, TS_WORDS * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  *total = (size_t)*reinterpret_cast<const unsigned int*>(m.nvox_h.h + 1);
  return NDT_OK;
}

// after map_export_count(sel, box) = total > 0: the selected slots compacted and ordered by ascending (k, j, i) -- output
// voxel r is table position (*slots)[(*order)[r]].  mn / mx: an ijk box that holds every selected voxel (the sort key is
// relative to it).  Enqueued, not awaited.
int map_export_order(ndt_handle* h, VoxelMap& m, const MapSel& sel, bool box_sel, size_t total, const int mn[3], const int mx[3],
                     const uint32_t** order_out, const uint32_t** slots_out) {
  hipStream_t s = h->stream;
  int rc = group_scratch(h, total, total + 1);
  if (rc) return rc;
  MapKeyBox box;
  for (int a = 0; a < 3; ++a) box.mn[a] = mn[a];
  box.bx = sort_key_bits((long long)mx[0] - mn[0]);
  box.by = sort_key_bits((long long)mx[1] - mn[1]);
  const int bits = box.bx + box.by + sort_key_bits((long long)mx[2] - mn[2]);
  const bool two_words = bits > 32;
  HIP_TRY(h, m.xslot.ensure(total));
  if (two_words) {
    HIP_TRY(h, m.xhi.ensure(total));
    HIP_TRY(h, m.xslot2.ensure(total));
  }
  const int nb = (int)((m.tab.capacity + MAP_XTILE - 1) / MAP_XTILE);
  if (box_sel)
    hipLaunchKernelGGL(k_map_xemit<true>, dim3((unsigned)nb), dim3(MAP_THREADS), 0, s, m.tab.keys, m.tab.cnt, (long long)m.tab.capacity, sel,
                       m.xcounts.p, box, m.xslot.p, h->sort.keys.p, two_words ? m.xhi.p : nullptr);
  else
    hipLaunchKernelGGL(k_map_xemit<false>, dim3((unsigned)nb), dim3(MAP_THREADS), 0, s, m.tab.keys, m.tab.cnt, (long long)m.tab.capacity, sel,
                       m.xcounts.p, box, m.xslot.p, h->sort.keys.p, two_words ? m.xhi.p : nullptr);
  HIP_TRY(h, hipGetLastError());
  int passes = 0;
  rc = sort_put_plan(h, h->gd.p, std::min(bits, 32), 0, &passes);
  if (rc) return rc;
  SortedPairs sorted;
  HIP_TRY(h, sort_keyed(h->sort, total, h->gd.p, passes, SORT_COUNT_FIRST, s, &sorted));
  const uint32_t* order = sorted.vals;
  const uint32_t* slots = m.xslot.p;
  if (two_words) {   // stable: the order of the low words survives among equal high words
    const unsigned tb = (unsigned)((total + MAP_THREADS - 1) / MAP_THREADS);
    hipLaunchKernelGGL(k_map_xgather, dim3(tb), dim3(MAP_THREADS), 0, s, order, m.xhi.p, m.xslot.p, (int)total, h->sort.keys.p, m.xslot2.p);
    HIP_TRY(h, hipGetLastError());
    rc = sort_put_plan(h, h->gd.p, bits - 32, 0, &passes);
    if (rc) return rc;
    HIP_TRY(h, sort_keyed(h->sort, total, h->gd.p, passes, SORT_COUNT_FIRST, s, &sorted));
    order = sorted.vals;
    slots = m.xslot2.p;
  }
  *order_out = order;
  *slots_out = slots;
  return NDT_OK;
}

namespace {

// after map_export_count(min_points) = total > 0: the first min(total, cap) voxels in ascending (k, j, i) order
int map_export_write(ndt_handle* h, int min_points, size_t total, float* ox, float* oy, float* oz, float* oi, int32_t* oc,
                     size_t cap) {
  VoxelMap& m = *h->map;
  hipStream_t s = h->stream;
  const size_t w = std::min(total, cap);
  if (w == 0) return NDT_OK;
  const uint32_t *order = nullptr, *slots = nullptr;
  int rc = map_export_order(h, m, sel_all(min_points), false, total, m.mn, m.mx, &order, &slots);
  if (rc) return rc;
  hipLaunchKernelGGL(k_map_xcentroids, dim3((unsigned)((w + MAP_THREADS - 1) / MAP_THREADS)), dim3(MAP_THREADS), 0, s, order, slots,
                     (int)w, m.tab.sums, m.tab.cnt, ox, oy, oz, m.with_intensity ? oi : nullptr, oc);
  HIP_TRY(h, hipGetLastError());
  if (oi && !m.with_intensity) HIP_TRY(h, hipMemsetAsync(oi, 0, w * sizeof(float), s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return NDT_OK;
}

}  // namespace

// the counters, read-back words and sort plans of a VoxelMap (the map's at ndt_map_reset, a level's at its first derivation)
int map_init_buffers(ndt_handle* h, VoxelMap& m) {
  hipError_t e = m.stats.ensure(MS_WORDS);
  if (e == hipSuccess) e = m.nvox.ensure(2);   // [1]: the voxels a re-pose creates in its fresh table
  if (e == hipSuccess) e = m.stats_h.ensure(2 * MS_WORDS);
  if (e == hipSuccess) e = m.nvox_h.ensure(2);
  if (e == hipSuccess) e = m.tsel.ensure(TS_WORDS);
  if (e == hipSuccess) e = m.tsel_h.ensure(2 * TS_WORDS);
  if (e == hipSuccess) e = hipMemsetAsync(m.nvox.p, 0, sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(h, e == hipErrorOutOfMemory ? NDT_ERR_ALLOC : NDT_ERR_HIP, hipGetErrorString(e));
  int* neutral = m.stats_h.h + MS_WORDS;
  for (int i = 0; i < MS_WORDS; ++i) neutral[i] = 0;
  for (int a = 0; a < 3; ++a) { neutral[MS_MIN + a] = INT_MAX; neutral[MS_MAX + a] = INT_MIN; }
  int* tneutral = m.tsel_h.h + TS_WORDS;
  for (int i = 0; i < TS_WORDS; ++i) tneutral[i] = 0;
  for (int a = 0; a < 3; ++a) { tneutral[TS_MIN + a] = INT_MAX; tneutral[TS_MAX + a] = INT_MIN; }
  return NDT_OK;
}

int no_map(ndt_handle* h) { return fail(h, NDT_ERR_INVALID_ARG, "no map (ndt_map_reset creates one)"); }

// floor(v * inv_leaf) in f32 as a point's voxel coordinate is, held to the map's coordinate range
int map_box_floor(float v, float inv_leaf) {
  const float f = floorf(v * inv_leaf);
  return f <= -MAP_LIMIT ? -MAP_BIAS : f >= MAP_LIMIT ? MAP_BIAS : (int)f;
}

bool pose_finite(const double p[16]) { return all_finite(p, 16); }

bool finite3(const float v[3]) { return all_finite(v, 3); }

int no_moments(ndt_handle* h) { return fail(h, NDT_ERR_INVALID_ARG, "the map keeps no moments (ndt_map_enable_moments right after ndt_map_reset)"); }

// ndt_set_target_from_map_moments behind its argument checks, on the map or on one of its levels (m.leaf is bit-equal to
// ndt_params::resolution).  Up to the one host wait nothing of the target is touched.
int target_from_moments(ndt_handle* h, VoxelMap& m, const float* box_min, const float* box_max) {
  settle_discard_keep_grid(h);   // (the pending build borrows the sort scratch; its verdict is dropped once this call replaces it)
  const auto t0 = std::chrono::steady_clock::now();
  MapSel sel{};
  sel.min_points = std::max(3, h->prm.min_points_per_voxel);  // the ordinary build's rule (build_begin)
  for (int a = 0; a < 3; ++a) {
    sel.lo[a] = box_min ? map_box_floor(box_min[a], m.inv_leaf) : -MAP_BIAS;
    sel.hi[a] = box_max ? map_box_floor(box_max[a], m.inv_leaf) : MAP_BIAS;
  }
  size_t total = 0;
  int rc = map_export_count(h, m, sel, true, &total);
  if (rc) return rc;
  const int* ts = m.tsel_h.h;
  if (m.n_voxels == 0 || ts[TS_VOXELS] == 0) return fail(h, NDT_ERR_NO_TARGET, "the map holds no occupied voxel inside the box");
  unsigned long long n_points = 0;
  std::memcpy(&n_points, ts + TS_POINTS, sizeof(n_points));
  int mn[3], mx[3];
  long long ncells = 1;
  const long long lim = std::numeric_limits<int32_t>::max();
  for (int a = 0; a < 3; ++a) {
    mn[a] = ts[TS_MIN + a];
    mx[a] = ts[TS_MAX + a];
    if (ncells < lim) ncells *= (long long)mx[a] - mn[a] + 1;   // (each factor <= 2^21: no overflow below the limit)
  }
  if (ncells >= lim)
    return fail(h, NDT_ERR_GRID_OVERFLOW, "the selected voxels span " + std::to_string(mx[0] - mn[0] + 1LL) + " x " +
                                              std::to_string(mx[1] - mn[1] + 1LL) + " x " + std::to_string(mx[2] - mn[2] + 1LL) +
                                              " cells (index overflow): select a box");
  if (total >= (size_t)lim) return fail(h, NDT_ERR_GRID_OVERFLOW, "too many leaves");

  // ---- from here on the target is replaced; no target points are retained ----
  hipStream_t s = h->stream;
  const IndexReuse reuse = target_retire(h, 0);

  // the dense grid: -1 everywhere once per allocation, afterwards only the previous build's cells are reset
  const size_t slots_needed = std::max<size_t>(total, 1);
  const bool steady = reuse.clean_cap != 0 && reuse.clean_cap == h->cell2leaf.cap && (size_t)ncells <= h->cell2leaf.cap &&
                      slots_needed <= h->stats.cap;
  if (steady) {
    if (reuse.dirty_slots > 0) {
      launch_reset_cells(h->stats.p, reuse.dirty_slots, h->cell2leaf.p, h->cell2leaf.cap, s);
      HIP_TRY(h, hipGetLastError());
    }
  } else {
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, h->cell2leaf.ensure((size_t)ncells));
    HIP_TRY(h, hipMemsetAsync(h->cell2leaf.p, 0xFF, h->cell2leaf.cap * sizeof(int), s));
    HIP_TRY(h, h->stats.ensure(slots_needed));
  }
  HIP_TRY(h, h->rec.ensure(slots_needed));
  HIP_TRY(h, h->cent.ensure(slots_needed * 4));

  const GridGeom g = grid_geom_from_box(h->prm.resolution, mn, mx);

  int n_valid = 0;
  if (total > 0) {
    const uint32_t *order = nullptr, *slots = nullptr;
    rc = map_export_order(h, m, sel, true, total, mn, mx, &order, &slots);
    if (rc) return rc;
    FinalizeParams fp{h->prm.eig_inflation_ratio, h->prm.cov_mode};
    launch_map_finalize(order, slots, total, m.tab.keys, m.tab.cnt, m.tab.mom, mn, g.mul1, g.mul2, fp, h->rec.p, h->cent.p, h->stats.p,
                        h->cell2leaf.p, m.tsel.p + TS_VALID, s);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(m.tsel_h.h + TS_VALID, m.tsel.p + TS_VALID, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    n_valid = m.tsel_h.h[TS_VALID];
  } else {
    // (geometry without a leaf: the evaluation reads record 0 for an absent neighbour, so it has to be finite)
    HIP_TRY(h, hipMemsetAsync(h->rec.p, 0, sizeof(VoxelRecord), s));
    HIP_TRY(h, hipStreamSynchronize(s));
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return target_publish(h, TargetKind::SINGLE, g, mx, (size_t)n_points, (int)total, n_valid, ms);
}

void map_release(ndt_handle* h) {
  if (!h->map) return;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  map_levels_release(h);
  h->map->release();
  delete h->map;
  h->map = nullptr;
}

}  // namespace engine
}  // namespace ndt

extern "C" {

int ndt_map_reset(ndt_handle* h, float leaf, int with_intensity, int64_t initial_capacity) {
  if (!h || !(leaf > 1e-6f) || !std::isfinite(leaf) || initial_capacity < 0 || initial_capacity > MAP_MAX_CAPACITY)
    return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  map_release(h);
  h->map = new VoxelMap();
  VoxelMap& m = *h->map;
  m.leaf = leaf;
  m.inv_leaf = 1.0f / leaf;
  m.with_intensity = with_intensity ? 1 : 0;
  const int64_t cap = map_pow2_at_least(initial_capacity > 0 ? initial_capacity : MAP_DEFAULT_CAPACITY);
  auto undo = [&](int code) { map_release(h); return code; };
  rc = map_alloc_table(h, cap, false, &m.tab);
  if (rc) return undo(rc);
  m.reset_capacity = cap;
  rc = map_init_buffers(h, m);
  if (rc) return undo(rc);
  return NDT_OK;
}

int ndt_map_clear(ndt_handle* h) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (!h->map) return NDT_OK;
  (void)hipSetDevice(h->device);
  map_release(h);
  return NDT_OK;
}

int ndt_map_add_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, const float* d_intensity, size_t n,
                       const double* pose16) {
  if (!h || ((!dx || !dy || !dz) && n)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  if (h->map->with_intensity && !d_intensity && n) return fail(h, NDT_ERR_INVALID_ARG, "the map keeps intensity: every add must bring it");
  if (pose16 && !pose_finite(pose16)) return fail(h, NDT_ERR_INVALID_ARG, "non-finite pose");
  return map_add_device(h, dx, dy, dz, d_intensity, n, pose16);
}

int ndt_map_add(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, long intensity_offset_bytes, const double* pose16) {
  if (!h || (!xyz && n) || !layout_valid(stride_bytes, intensity_offset_bytes)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  VoxelMap& m = *h->map;
  const bool has_i = m.with_intensity != 0;
  if (has_i && intensity_offset_bytes < 0) return fail(h, NDT_ERR_INVALID_ARG, "the map keeps intensity: every add must bring it");
  if (pose16 && !pose_finite(pose16)) return fail(h, NDT_ERR_INVALID_ARG, "non-finite pose");
  if (n == 0) return NDT_OK;
  settle_discard_keep_grid(h);
  rc = upload_soa(h, h->lane_t, h->stream, xyz, nullptr, nullptr, nullptr, n, stride_bytes, m.ux, m.uy, m.uz, true);
  if (rc) return rc;
  if (has_i) {
    rc = upload_column(h, xyz, n, stride_bytes, (size_t)intensity_offset_bytes, m.ui);
    if (rc) return rc;
  }
  return map_add_device(h, m.ux.p, m.uy.p, m.uz.p, has_i ? m.ui.p : nullptr, n, pose16);
}

int ndt_map_add_keyframe(ndt_handle* h, int64_t id, const double pose16[16]) {
  if (!h || !pose16) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  if (h->map->with_intensity) return fail(h, NDT_ERR_INVALID_ARG, "the map keeps intensity: the keyframe archive holds xyz only");
  if (!pose_finite(pose16)) return fail(h, NDT_ERR_INVALID_ARG, "non-finite pose");
  auto it = h->keyframes.find(id);
  if (it == h->keyframes.end()) return fail(h, NDT_ERR_INVALID_ARG, "unknown keyframe id");
  const ndt_handle::Keyframe& kf = it->second;
  return map_add_device(h, kf.x.p, kf.y.p, kf.z.p, nullptr, kf.n, pose16);
}

int ndt_map_get_info(const ndt_handle* h, ndt_map_info* out) {
  if (!h || !out) return NDT_ERR_INVALID_ARG;
  if (!h->map) return NDT_ERR_INVALID_ARG;
  VoxelMap& m = *h->map;
  if (m.nvox_stale) {   // (every add returns with its launches complete: a plain copy)
    (void)hipSetDevice(h->device);
    if (hipMemcpy(m.nvox_h.h, m.nvox.p, sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return NDT_ERR_HIP;
    m.n_voxels = (int64_t)m.nvox_h.h[0];
    m.nvox_stale = false;
  }
  *out = ndt_map_info{};
  out->leaf = m.leaf;
  out->with_intensity = m.with_intensity;
  out->n_voxels = m.n_voxels;
  out->n_points = m.n_points;
  out->n_points_dropped = m.n_dropped;
  out->capacity = m.tab.capacity;
  for (int a = 0; a < 3; ++a) { out->min_ijk[a] = m.mn[a]; out->max_ijk[a] = m.mx[a]; }
  out->n_adds = m.n_adds;
  out->n_grows = m.n_grows;
  return NDT_OK;
}

int ndt_map_export_device(ndt_handle* h, int min_points, float* ox, float* oy, float* oz, float* o_intensity, int32_t* o_count,
                          size_t cap, size_t* n_out) {
  if (!h || !n_out || ((!ox || !oy || !oz) && cap)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  settle_discard_keep_grid(h);
  size_t total = 0;
  rc = map_export_count(h, *h->map, sel_all(min_points), false, &total);
  if (rc) return rc;
  *n_out = total;
  if (total == 0) return NDT_OK;
  rc = map_export_write(h, min_points, total, ox, oy, oz, o_intensity, o_count, cap);
  if (rc) return rc;
  if (total > cap) return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(total) + " voxels");
  return NDT_OK;
}

int ndt_map_export(ndt_handle* h, int min_points, float* out, size_t stride_bytes, long intensity_offset_bytes, int32_t* count_out,
                   size_t cap, size_t* n_out) {
  if (!h || !n_out || (!out && cap) || !layout_valid(stride_bytes, intensity_offset_bytes)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  VoxelMap& m = *h->map;
  settle_discard_keep_grid(h);
  size_t total = 0;
  rc = map_export_count(h, *h->map, sel_all(min_points), false, &total);
  if (rc) return rc;
  *n_out = total;
  if (total == 0) return NDT_OK;
  const size_t w = std::min(total, cap);   // the voxels that fit are written, a shortfall is reported behind them
  if (w) {
    HIP_TRY(h, m.xout.ensure(4 * w));
    HIP_TRY(h, m.xcnt.ensure(w));
    float* o = m.xout.p;
    rc = map_export_write(h, min_points, total, o, o + w, o + 2 * w, intensity_offset_bytes >= 0 ? o + 3 * w : nullptr, m.xcnt.p, w);
    if (rc) return rc;
    SideColumns counts;
    counts.d_i32 = m.xcnt.p;
    counts.i32_out = count_out;
    rc = download_strided(h, o, w, w, w, out, stride_bytes, intensity_offset_bytes, nullptr, counts);
    if (rc) return rc;
  }
  if (total > cap) return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(total) + " voxels");
  return NDT_OK;
}

int ndt_set_target_from_map(ndt_handle* h, int min_points) {
  if (!h) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  settle_discard(h);
  size_t total = 0;
  rc = map_export_count(h, *h->map, sel_all(min_points), false, &total);
  if (rc) return rc;
  if (total == 0) return fail(h, NDT_ERR_NO_TARGET, "the map holds no voxel with that many points");
  h->tgt.claim_cloud();
  HIP_TRY(h, h->tx.ensure(total));
  HIP_TRY(h, h->ty.ensure(total));
  HIP_TRY(h, h->tz.ensure(total));
  rc = map_export_write(h, min_points, total, h->tx.p, h->ty.p, h->tz.p, nullptr, nullptr, total);
  if (rc) return rc;
  // (the centroids are the engine's own: the build may stay in flight like a host hand-off's)
  return build_grid(h, h->tx.p, h->ty.p, h->tz.p, total, h->handoff_mode == NDT_HANDOFF_ASYNC);
}

int ndt_map_enable_moments(ndt_handle* h) {
  if (!h) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  VoxelMap& m = *h->map;
  if (m.moments) return fail(h, NDT_ERR_INVALID_ARG, "the map keeps moments already");
  if (m.n_points > 0 || m.n_voxels > 0 || m.nvox_stale)
    return fail(h, NDT_ERR_INVALID_ARG, "the map holds points already: moments are enabled right after ndt_map_reset");
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&m.tab.mom), (size_t)m.tab.capacity * 9 * sizeof(double));
  if (e == hipSuccess) e = hipMemsetAsync(m.tab.mom, 0, (size_t)m.tab.capacity * 9 * sizeof(double), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (m.tab.mom) (void)hipFree(m.tab.mom);
    m.tab.mom = nullptr;
    return fail(h, e == hipErrorOutOfMemory ? NDT_ERR_ALLOC : NDT_ERR_HIP, std::string("voxel map moments: ") + hipGetErrorString(e));
  }
  m.moments = true;
  ++m.change;
  return NDT_OK;
}

int ndt_map_has_moments(const ndt_handle* h) {
  if (!h) return NDT_ERR_INVALID_ARG;
  return h->map && h->map->moments ? 1 : 0;
}

int ndt_map_export_moments(ndt_handle* h, int min_points, int32_t* ijk, int32_t* count, double* sums, size_t cap, size_t* n_out) {
  if (!h || !n_out) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  VoxelMap& m = *h->map;
  if (!m.moments) return no_moments(h);
  settle_discard_keep_grid(h);
  size_t total = 0;
  rc = map_export_count(h, *h->map, sel_all(min_points), false, &total);
  if (rc) return rc;
  *n_out = total;
  if (total == 0) return NDT_OK;
  const size_t w = std::min(total, cap);
  if (w && (ijk || count || sums)) {
    HIP_TRY(h, m.xijk.ensure(3 * w));
    HIP_TRY(h, m.xcnt.ensure(w));
    HIP_TRY(h, m.xmom.ensure(9 * w));
    const uint32_t *order = nullptr, *slots = nullptr;
    rc = map_export_order(h, m, sel_all(min_points), false, total, m.mn, m.mx, &order, &slots);
    if (rc) return rc;
    launch_map_gather_moments(order, slots, w, m.tab.keys, m.tab.cnt, m.tab.mom, m.xijk.p, m.xcnt.p, m.xmom.p, h->stream);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (ijk) HIP_TRY(h, hipMemcpy(ijk, m.xijk.p, 3 * w * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (count) HIP_TRY(h, hipMemcpy(count, m.xcnt.p, w * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (sums) HIP_TRY(h, hipMemcpy(sums, m.xmom.p, 9 * w * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (total > cap) return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(total) + " voxels");
  return NDT_OK;
}

int ndt_set_target_from_map_moments(ndt_handle* h, const float box_min[3], const float box_max[3]) {
  if (!h || (box_min == nullptr) != (box_max == nullptr)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  VoxelMap& m = *h->map;
  if (!m.moments) return no_moments(h);
  if (std::memcmp(&m.leaf, &h->prm.resolution, sizeof(float)) != 0)
    return fail(h, NDT_ERR_INVALID_ARG, "the map's leaf size is not ndt_params::resolution: a voxel of the map is not a voxel of the grid");
  if (box_min && !(finite3(box_min) && finite3(box_max))) return fail(h, NDT_ERR_INVALID_ARG, "non-finite box");
  return target_from_moments(h, m, box_min, box_max);
}

}  // extern "C"
