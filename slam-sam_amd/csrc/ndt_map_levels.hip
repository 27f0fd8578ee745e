// ndt_map_levels.hip -- the voxel map at leaf * 2^L, made from its own sums (ndt_map_level_*, ndt_set_target_from_map_level,
// ndt_map_coarsen, ndt_align_map_levels; the rule is stated in include/ndt_hip.h).  A level is a VoxelMap of its own
// (ndt_handle::map_level), so the export, the box selection and the target build of ndt_map.hip / ndt_map_state.hip run on
// it as they run on the map.
//   derive   the map's occupied voxels in ascending (k, j, i) order (map_export_order) -> k_maplevel_keys: the parent's key
//            per ordered voxel (ijk >> L, re-packed by the one codec) and the voxel's table position -> the add's insert into
//            a fresh table, stable sort of (slot, order index) and run search (map_group_batch) -> k_maplevel_accumulate:
//            one lane per level voxel gathers its children from the map's table in that order, every field from +0, one
//            rounding per add (ONE host wait: the level's voxel count, tight ijk box, point total and the overflow verdict)
// No record is materialised and nothing passes through the host.  The rules of ndt_map.hip hold: wave64, integer atomics
// only (one per word and block; the overflow flag is one per offending voxel, normally none), no float atomics, no tree
// within a field, no kernel waits for another block.
#include "ndt_engine.h"
#include "ndt_map_device.h"

namespace ndt {

namespace {

// Ordered fine voxel r (table position slots[order[r]]): its parent's key at `shift` levels up and its own position.  The
// statistics of the batch -- the parents' ijk box and the 64-bit point total -- go to `stats` as an import's do.
__global__ void __launch_bounds__(MAP_THREADS) k_maplevel_keys(const uint32_t* __restrict__ order, const uint32_t* __restrict__ slots,
                                                              int n, const unsigned long long* __restrict__ tkeys,
                                                              const int* __restrict__ cnt, int shift,
                                                              unsigned long long* __restrict__ pkey, uint32_t* __restrict__ child,
                                                              int* __restrict__ stats) {
  const int r = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  unsigned long long pts = 0;
  if (r < n) {
    const uint32_t slot = slots[order[r]];
    int v[3];
    map_ijk(tkeys[slot], v);
#pragma unroll
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = v[a] >> shift;   // (arithmetic: floor_div by 2^shift)
    pts = (unsigned long long)cnt[slot];
    pkey[r] = map_key(mn[0], mn[1], mn[2]);
    child[r] = slot;
  }
  map_record_stats(0, 0, pts, mn, mx, stats);
}

// Run r of the slot-sorted batch = the children vals_sorted[start .. start + cnt) of one level voxel in ascending fine
// (k, j, i) order (the radix sort is stable): every field from +0, one child at a time, one rounding per add (built with
// -ffp-contract=off; there is no product to contract anyway).  The count is summed in 64 bits: a voxel beyond INT32_MAX
// is counted in stats[MS_BAD_COUNT] and the host refuses the level.
template <bool MOM>
__global__ void __launch_bounds__(MAP_THREADS) k_maplevel_accumulate(const int* __restrict__ d_nleaf, const int* __restrict__ leaf_start,
                                                                    const int* __restrict__ leaf_cnt,
                                                                    const uint32_t* __restrict__ keys_sorted,
                                                                    const uint32_t* __restrict__ vals_sorted,
                                                                    const uint32_t* __restrict__ child,
                                                                    const float4* __restrict__ bsums, const int* __restrict__ bcnt,
                                                                    const double* __restrict__ bmom, int with_intensity,
                                                                    float4* __restrict__ sums, int* __restrict__ cnt,
                                                                    double* __restrict__ mom, int* __restrict__ stats) {
  const int r = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  if (r >= d_nleaf[0]) return;
  const int start = leaf_start[r], c = leaf_cnt[r];
  const uint32_t slot = keys_sorted[start];
  float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  long long total = 0;
  double q[9];
  if (MOM) {
#pragma unroll
    for (int a = 0; a < 9; ++a) q[a] = 0.0;
  }
  for (int j = 0; j < c; ++j) {
    const size_t p = child[vals_sorted[start + j]];
    const float4 b = bsums[p];
    s.x += b.x; s.y += b.y; s.z += b.z;
    if (with_intensity) s.w += b.w;
    total += (long long)bcnt[p];
    if (MOM) {
#pragma unroll
      for (int a = 0; a < 9; ++a) q[a] += bmom[p * 9 + a];
    }
  }
  if (total > (long long)INT_MAX) {
    atomicAdd(stats + MS_BAD_COUNT, 1);
    total = INT_MAX;
  }
  sums[slot] = s;
  cnt[slot] = (int)total;
  if (MOM) {
#pragma unroll
    for (int a = 0; a < 9; ++a) mom[(size_t)slot * 9 + a] = q[a];
  }
}

}  // namespace

namespace engine {

void map_levels_release(ndt_handle* h) {
  for (VoxelMap*& lv : h->map_level) {
    if (!lv) continue;
    lv->release();
    delete lv;
    lv = nullptr;
  }
}

namespace {

int bad_level(ndt_handle* h) {
  return fail(h, NDT_ERR_INVALID_ARG, "level outside 0 .. " + std::to_string(NDT_MAP_MAX_LEVEL));
}

// (float)(leaf * 2^L): exact in f32 unless it overflows
float level_leaf(const VoxelMap& b, int level) { return b.leaf * (float)(1 << level); }

int drop_level(ndt_handle* h, VoxelMap* lv, int rc) {
  (void)hipStreamSynchronize(h->stream);   // (what the derivation enqueued may still write to it)
  (void)hipGetLastError();
  lv->release();
  delete lv;
  return rc;
}

// The level's VoxelMap, derived if the cache does not hold it for the map's present content.  Refusals leave the cache
// without that level and everything else as it was.
int level_get(ndt_handle* h, int level, VoxelMap** out) {
  VoxelMap& b = *h->map;
  *out = nullptr;
  if (level < 0 || level > NDT_MAP_MAX_LEVEL) return bad_level(h);
  if (level == 0) { *out = &b; return NDT_OK; }
  const float leaf = level_leaf(b, level);
  if (!std::isfinite(leaf)) return fail(h, NDT_ERR_INVALID_ARG, "the level's leaf size is not finite");
  VoxelMap*& cached = h->map_level[level - 1];
  if (cached && cached->derived_at == b.change) { *out = cached; return NDT_OK; }
  settle_discard_keep_grid(h);   // (a pending build borrows the sort scratch)
  hipStream_t s = h->stream;
  if (cached) {   // stale (every call that used it has completed)
    cached->release();
    delete cached;
    cached = nullptr;
  }
  int rc = map_refresh_voxel_count(h, b);
  if (rc) return rc;
  VoxelMap* lv = new VoxelMap();
  lv->leaf = leaf;
  lv->inv_leaf = 1.0f / leaf;
  lv->with_intensity = b.with_intensity;
  rc = map_init_buffers(h, *lv);
  if (rc) return drop_level(h, lv, rc);
  lv->moments = b.moments;   // (behind the buffers: release() clears it)
  const size_t n = (size_t)b.n_voxels;
  if (n > 0) {
    if (n > (size_t)std::numeric_limits<int>::max() / 2) return drop_level(h, lv, fail(h, NDT_ERR_INVALID_ARG, "too many voxels for one level"));
    const int64_t cap = map_pow2_at_least(2 * (int64_t)n);
    if (cap > MAP_MAX_CAPACITY) return drop_level(h, lv, fail(h, NDT_ERR_ALLOC, "voxel map level: more than 2^30 table slots needed"));
    hipError_t e = lv->pkey.ensure(n);
    if (e == hipSuccess) e = lv->lchild.ensure(n);
    if (e != hipSuccess) return drop_level(h, lv, fail(h, e == hipErrorOutOfMemory ? NDT_ERR_ALLOC : NDT_ERR_HIP, hipGetErrorString(e)));
    rc = group_scratch(h, n, n + 1);
    if (rc) return drop_level(h, lv, rc);
    MapSel sel{};
    sel.min_points = INT_MIN;   // every occupied voxel
    size_t total = 0;
    rc = map_export_count(h, b, sel, false, &total);
    if (rc) return drop_level(h, lv, rc);
    if (total != n)
      return drop_level(h, lv, fail(h, NDT_ERR_HIP, "voxel map level: the table holds " + std::to_string(total) + " voxels, the counter says " + std::to_string(n)));
    // the level's (so far absent) table is replaced by a fresh one that the derivation fills: the one way a table comes
    // to be (map_grow_table with a refill, as the re-pose does), which counts the voxels created and awaits the stream
    const MapRefill refill{"voxel map level: ", [&](const MapTable& fresh) {
      const uint32_t *order = nullptr, *slots = nullptr;
      int r = map_export_order(h, b, sel, false, total, b.mn, b.mx, &order, &slots);
      if (r) return r;
      const unsigned blocks = (unsigned)((n + MAP_THREADS - 1) / MAP_THREADS);
      HIP_TRY(h, hipMemcpyAsync(lv->stats.p, lv->stats_h.h + MS_WORDS, MS_WORDS * sizeof(int), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_maplevel_keys, dim3(blocks), dim3(MAP_THREADS), 0, s, order, slots, (int)n, b.tab.keys, b.tab.cnt, level,
                         lv->pkey.p, lv->lchild.p, lv->stats.p);
      HIP_TRY(h, hipGetLastError());
      const uint32_t *keys_sorted = nullptr, *vals_sorted = nullptr;
      r = map_group_batch(h, *lv, n, fresh, lv->nvox.p + 1, &keys_sorted, &vals_sorted);
      if (r) return r;
      if (b.moments)
        hipLaunchKernelGGL(k_maplevel_accumulate<true>, dim3(blocks), dim3(MAP_THREADS), 0, s, h->nleaf.p, h->leaf_start.p, h->leaf_cnt.p,
                           keys_sorted, vals_sorted, lv->lchild.p, b.tab.sums, b.tab.cnt, b.tab.mom, b.with_intensity, fresh.sums,
                           fresh.cnt, fresh.mom, lv->stats.p);
      else
        hipLaunchKernelGGL(k_maplevel_accumulate<false>, dim3(blocks), dim3(MAP_THREADS), 0, s, h->nleaf.p, h->leaf_start.p, h->leaf_cnt.p,
                           keys_sorted, vals_sorted, lv->lchild.p, b.tab.sums, b.tab.cnt, static_cast<const double*>(nullptr),
                           b.with_intensity, fresh.sums, fresh.cnt, static_cast<double*>(nullptr), lv->stats.p);
      HIP_TRY(h, hipGetLastError());
      HIP_TRY(h, hipMemcpyAsync(lv->stats_h.h, lv->stats.p, MS_WORDS * sizeof(int), hipMemcpyDeviceToHost, s));
      return (int)NDT_OK;
    }};
    rc = map_grow_table(h, *lv, cap, &refill);   // the derivation's one host wait; n_voxels is the count of voxels created
    if (rc) return drop_level(h, lv, rc);
    const int* st = lv->stats_h.h;
    if (st[MS_PROBE_FAIL] > 0) return drop_level(h, lv, fail(h, NDT_ERR_HIP, "voxel map level: a voxel found no table position"));
    if (st[MS_BAD_COUNT] > 0)
      return drop_level(h, lv, fail(h, NDT_ERR_GRID_OVERFLOW, std::to_string(st[MS_BAD_COUNT]) + " level voxel(s) would hold more than INT32_MAX points; the level is refused"));
    unsigned long long pts = 0;
    std::memcpy(&pts, st + MS_POINTS, sizeof(pts));
    lv->n_points = (int64_t)pts;
    for (int a = 0; a < 3; ++a) { lv->mn[a] = st[MS_MIN + a]; lv->mx[a] = st[MS_MAX + a]; }
    lv->lchild.release();   // (the derivation's own)
    lv->pkey.release();
  }
  lv->derived_at = b.change;
  cached = lv;
  *out = lv;
  return NDT_OK;
}

int level_entry(ndt_handle* h) {
  const int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  return NDT_OK;
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

int ndt_map_level_info(ndt_handle* h, int level, ndt_map_info* out) {
  if (!h || !out) return NDT_ERR_INVALID_ARG;
  int rc = level_entry(h);
  if (rc) return rc;
  if (level == 0) return ndt_map_get_info(h, out);
  VoxelMap* lv = nullptr;
  rc = level_get(h, level, &lv);
  if (rc) return rc;
  const VoxelMap& b = *h->map;
  *out = ndt_map_info{};
  out->leaf = lv->leaf;
  out->with_intensity = lv->with_intensity;
  out->n_voxels = lv->n_voxels;
  out->n_points = lv->n_points;
  out->n_points_dropped = b.n_dropped;
  out->capacity = lv->tab.capacity;
  for (int a = 0; a < 3; ++a) { out->min_ijk[a] = lv->mn[a]; out->max_ijk[a] = lv->mx[a]; }
  out->n_adds = b.n_adds;
  out->n_grows = b.n_grows;
  return NDT_OK;
}

int ndt_map_export_state_level_device(ndt_handle* h, int level, const float box_min[3], const float box_max[3], int32_t* ijk,
                                      int32_t* count, float* sums4, double* moments9, size_t cap, size_t* n_out) {
  if (!h || !n_out || (box_min == nullptr) != (box_max == nullptr)) return NDT_ERR_INVALID_ARG;
  int rc = level_entry(h);
  if (rc) return rc;
  VoxelMap* lv = nullptr;
  rc = level_get(h, level, &lv);
  if (rc) return rc;
  return map_export_state_public(h, *lv, true, box_min, box_max, ijk, count, sums4, moments9, cap, n_out);
}

int ndt_map_export_state_level(ndt_handle* h, int level, const float box_min[3], const float box_max[3], int32_t* ijk,
                               int32_t* count, float* sums4, double* moments9, size_t cap, size_t* n_out) {
  if (!h || !n_out || (box_min == nullptr) != (box_max == nullptr)) return NDT_ERR_INVALID_ARG;
  int rc = level_entry(h);
  if (rc) return rc;
  VoxelMap* lv = nullptr;
  rc = level_get(h, level, &lv);
  if (rc) return rc;
  return map_export_state_public(h, *lv, false, box_min, box_max, ijk, count, sums4, moments9, cap, n_out);
}

int ndt_set_target_from_map_level(ndt_handle* h, int level, const float box_min[3], const float box_max[3]) {
  if (!h || (box_min == nullptr) != (box_max == nullptr)) return NDT_ERR_INVALID_ARG;
  if (level == 0) return ndt_set_target_from_map_moments(h, box_min, box_max);
  int rc = level_entry(h);
  if (rc) return rc;
  VoxelMap& b = *h->map;
  if (level < 0 || level > NDT_MAP_MAX_LEVEL) return bad_level(h);
  if (!b.moments) return no_moments(h);
  const float leaf = level_leaf(b, level);
  if (std::memcmp(&leaf, &h->prm.resolution, sizeof(float)) != 0)
    return fail(h, NDT_ERR_INVALID_ARG, "the level's leaf size is not ndt_params::resolution: a voxel of the level is not a voxel of the grid");
  if (box_min && !(finite3(box_min) && finite3(box_max))) return fail(h, NDT_ERR_INVALID_ARG, "non-finite box");
  VoxelMap* lv = nullptr;
  rc = level_get(h, level, &lv);
  if (rc) return rc;
  return target_from_moments(h, *lv, box_min, box_max);
}

int ndt_map_levels_drop(ndt_handle* h) {
  if (!h) return NDT_ERR_INVALID_ARG;
  const int rc = level_entry(h);
  if (rc) return rc;
  (void)hipStreamSynchronize(h->stream);
  map_levels_release(h);
  return NDT_OK;
}

int ndt_map_coarsen(ndt_handle* h, int level) {
  if (!h) return NDT_ERR_INVALID_ARG;
  int rc = level_entry(h);
  if (rc) return rc;
  VoxelMap* lv = nullptr;
  rc = level_get(h, level, &lv);
  if (rc) return rc;
  if (level == 0) return NDT_OK;
  VoxelMap& b = *h->map;
  if (lv->tab.capacity) {   // (a level of an empty map has no table: the map keeps its own, empty one)
    b.nvox_h.h[0] = (unsigned long long)lv->n_voxels;
    HIP_TRY(h, hipMemcpy(b.nvox.p, b.nvox_h.h, sizeof(unsigned long long), hipMemcpyHostToDevice));   // the next add reads the device's counter
    map_free_table(b.tab);
    b.tab = lv->tab;
    lv->tab = MapTable{};
    b.n_voxels = lv->n_voxels;
    b.nvox_stale = false;
    for (int a = 0; a < 3; ++a) { b.mn[a] = lv->mn[a]; b.mx[a] = lv->mx[a]; }
  }
  b.leaf = lv->leaf;
  b.inv_leaf = lv->inv_leaf;
  ++b.change;
  map_levels_release(h);
  return NDT_OK;
}

int ndt_align_map_levels(ndt_handle* h, const ndt_map_level_step* steps, int n_steps, const float half_extent_or_null[3],
                         const float guess_colmajor[16], ndt_result* results) {
  if (!h || !steps || !guess_colmajor || !results || n_steps < 1 || n_steps > NDT_MAP_LEVEL_STEPS_MAX) return NDT_ERR_INVALID_ARG;
  int rc = level_entry(h);
  if (rc) return rc;
  if (half_extent_or_null && !finite3(half_extent_or_null)) return fail(h, NDT_ERR_INVALID_ARG, "non-finite half extent");
  const ndt_params saved = h->prm;
  float guess[16];
  std::memcpy(guess, guess_colmajor, sizeof(guess));
  for (int s = 0; s < n_steps && rc == NDT_OK; ++s) {
    const ndt_map_level_step& st = steps[s];
    if (st.level < 0 || st.level > NDT_MAP_MAX_LEVEL) { rc = bad_level(h); break; }
    ndt_params p = saved;
    p.resolution = level_leaf(*h->map, st.level);
    if (st.max_iterations != 0) p.max_iterations = st.max_iterations;
    if (st.step_size != 0.0) p.step_size = st.step_size;
    rc = ndt_set_params(h, &p);
    if (rc) break;
    if (half_extent_or_null) {
      float lo[3], hi[3];
      for (int a = 0; a < 3; ++a) { lo[a] = guess[12 + a] - half_extent_or_null[a]; hi[a] = guess[12 + a] + half_extent_or_null[a]; }
      rc = ndt_set_target_from_map_level(h, st.level, lo, hi);
    } else {
      rc = ndt_set_target_from_map_level(h, st.level, nullptr, nullptr);
    }
    if (rc) break;
    rc = ndt_align(h, guess, &results[s]);
    if (rc) break;
    std::memcpy(guess, results[s].final_transformation, sizeof(guess));
  }
  // the caller's parameters again, whatever happened (the failing step's message stays)
  const std::string err = h->err;
  const int rc2 = ndt_set_params(h, &saved);
  if (rc) { h->err = err; return rc; }
  return rc2;
}

}  // extern "C"
