// ndt_map_state.hip -- the voxel map beyond add and export (ndt_map.hip, see ndt_engine.h: VoxelMap): remove voxels by
// box, hand out and take back the complete per-voxel state, merge one map into another.
//   crop     the export's count pass under the box predicate (ONE host wait: how many voxels and points the box holds
//            decides whether anything moves and sizes the new table) -> the survivors move to a fresh table as growth moves
//            them, the same launch reducing their tight ijk box -> the device's voxel counter is set to what was kept
//   export   the export's count / scan / compaction / key sort under the box predicate, the key relative to the ijk box
//            of the selection -> one gather: ijk, count, the four float sums and the nine f64 sums as the table holds them
//   import   keys from the records' ijk + range / count check (ONE host wait: refusal / growth are decided before anything
//            is written) -> the add's insert, stable sort of (slot, record index) and run search -> one thread per run
//            continues the voxel's sums with the run's records in input order: field = old + record.field, one rounding
// A fresh slot holds +0 in every field and 0 + s == s bit for bit for every s but -0.0, which a map never holds (its
// sums start at +0, and +0 + x is -0 for no x; x + y is -0 only for x = y = -0): a voxel new to the map receives its
// record exactly, and export -> import into an empty map reproduces the table's content.
// The import behind its key pass (map_import_tail) and the merge into a given table (map_merge_records) also serve the
// re-pose of ndt_map_repose.hip, whose record pass stands in for k_mapstate_keys; both share map_record_stats.
// The rules of ndt_map.hip hold: wave64, integer atomics only (one per word and block), no kernel waits for another
// block, every probe loop is bounded by the capacity.
#include "ndt_engine.h"
#include "ndt_map_device.h"

namespace ndt {

namespace {

// Crop: every occupied slot of the old table whose voxel is inside the box (remove_inside == 0) or outside it
// (remove_inside != 0) moves to the new table (map_move_slot); the survivors' ijk box goes to tsel (TS_MIN / TS_MAX).
__global__ void __launch_bounds__(MAP_THREADS) k_mapstate_crop(MapTable o, MapSel sel, int remove_inside, MapTable t,
                                                              int* __restrict__ stats, int* __restrict__ tsel) {
  __shared__ int box[MAP_WAVES][6];
  const long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  if (i < o.capacity) {
    const unsigned long long key = o.keys[i];
    if (key != MAP_EMPTY && map_in_box(key, sel) == (remove_inside == 0) && map_move_slot(o, i, key, t, stats)) {
      map_ijk(key, mn);
      map_ijk(key, mx);
    }
  }
  map_box_waves(mn, mx, box);
  __syncthreads();
  map_box_commit(box, tsel + TS_MIN, tsel + TS_MAX);
}

// output record r = the voxel slots[order[r]] as the table holds it: absolute ijk, count, the four float sums (NOT
// divided), the nine f64 sums.  Any output may be null (omom only where the table has moments).
__global__ void __launch_bounds__(MAP_THREADS) k_mapstate_gather(const uint32_t* __restrict__ order, const uint32_t* __restrict__ slots,
                                                                int m, const unsigned long long* __restrict__ tkeys,
                                                                const float4* __restrict__ sums, const int* __restrict__ cnt,
                                                                const double* __restrict__ mom, int32_t* __restrict__ oijk,
                                                                int32_t* __restrict__ ocount, float* __restrict__ osums,
                                                                double* __restrict__ omom) {
  const int r = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  if (r >= m) return;
  const uint32_t slot = slots[order[r]];
  if (oijk) {
    int v[3];
    map_ijk(tkeys[slot], v);
    oijk[(size_t)r * 3 + 0] = v[0]; oijk[(size_t)r * 3 + 1] = v[1]; oijk[(size_t)r * 3 + 2] = v[2];
  }
  if (ocount) ocount[r] = cnt[slot];
  if (osums) {   // (the caller's array need not be 16-byte aligned)
    const float4 s = sums[slot];
    osums[(size_t)r * 4 + 0] = s.x; osums[(size_t)r * 4 + 1] = s.y; osums[(size_t)r * 4 + 2] = s.z; osums[(size_t)r * 4 + 3] = s.w;
  }
  if (omom) {
#pragma unroll
    for (int a = 0; a < 9; ++a) omom[(size_t)r * 9 + a] = mom[(size_t)slot * 9 + a];
  }
}

// Voxel key per record, from its ijk (k_map_keys' packing).  MAP_EMPTY for a record outside the coordinate range or with
// count < 1 (both counted: the host refuses the whole import).  The batch's statistics -- those two numbers, the ijk box
// and the 64-bit point total of the valid records -- go to `stats` with one integer atomic per word and block.
__global__ void __launch_bounds__(MAP_THREADS) k_mapstate_keys(const int32_t* __restrict__ ijk, const int32_t* __restrict__ count,
                                                              int n, unsigned long long* __restrict__ pkey,
                                                              int* __restrict__ stats) {
  const int i = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  int oor = 0, bad = 0;
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  unsigned long long pts = 0;
  if (i < n) {
    const int vi = ijk[(size_t)i * 3 + 0], vj = ijk[(size_t)i * 3 + 1], vk = ijk[(size_t)i * 3 + 2];
    const int c = count[i];
    unsigned long long key = MAP_EMPTY;
    const bool in_range = vi > -MAP_BIAS && vi < MAP_BIAS && vj > -MAP_BIAS && vj < MAP_BIAS && vk > -MAP_BIAS && vk < MAP_BIAS;
    if (!in_range) oor = 1;
    if (c < 1) bad = 1;
    if (in_range && c >= 1) {
      mn[0] = mx[0] = vi; mn[1] = mx[1] = vj; mn[2] = mx[2] = vk;
      pts = (unsigned long long)c;
      key = map_key(vi, vj, vk);
    }
    pkey[i] = key;
  }
  map_record_stats(oor, bad, pts, mn, mx, stats);
}

// Run r of the slot-sorted batch = records vals_sorted[start .. start + cnt) of one voxel, in input order (the radix sort
// is stable): every field of the slot goes on from what the map holds, one record at a time, old + record.field (built
// with -ffp-contract=off; there is no product to contract anyway).  A fresh slot holds +0 everywhere.
template <bool MOM>
__global__ void __launch_bounds__(MAP_THREADS) k_mapstate_accumulate(const int* __restrict__ d_nleaf, const int* __restrict__ leaf_start,
                                                                    const int* __restrict__ leaf_cnt,
                                                                    const uint32_t* __restrict__ keys_sorted,
                                                                    const uint32_t* __restrict__ vals_sorted,
                                                                    const int32_t* __restrict__ rcount, const float* __restrict__ rsums,
                                                                    const double* __restrict__ rmom, int with_intensity,
                                                                    float4* __restrict__ sums, int* __restrict__ cnt,
                                                                    double* __restrict__ mom) {
  const int r = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  if (r >= d_nleaf[0]) return;
  const int start = leaf_start[r], c = leaf_cnt[r];
  const uint32_t slot = keys_sorted[start];
  float4 s = sums[slot];
  int total = cnt[slot];
  double q[9];
  if (MOM) {
#pragma unroll
    for (int a = 0; a < 9; ++a) q[a] = mom[(size_t)slot * 9 + a];
  }
  for (int j = 0; j < c; ++j) {
    const size_t p = vals_sorted[start + j];
    s.x += rsums[p * 4 + 0]; s.y += rsums[p * 4 + 1]; s.z += rsums[p * 4 + 2];
    if (with_intensity) s.w += rsums[p * 4 + 3];
    total += rcount[p];
    if (MOM) {
#pragma unroll
      for (int a = 0; a < 9; ++a) q[a] += rmom[p * 9 + a];
    }
  }
  sums[slot] = s;
  cnt[slot] = total;
  if (MOM) {
#pragma unroll
    for (int a = 0; a < 9; ++a) mom[(size_t)slot * 9 + a] = q[a];
  }
}

}  // namespace

namespace engine {
namespace {

// the selection of a box (both corners null: the whole coordinate range), whatever the voxels' counts
MapSel sel_box(const VoxelMap& m, const float* box_min, const float* box_max) {
  MapSel sel{};
  sel.min_points = INT_MIN;
  for (int a = 0; a < 3; ++a) {
    sel.lo[a] = box_min ? map_box_floor(box_min[a], m.inv_leaf) : -MAP_BIAS;
    sel.hi[a] = box_max ? map_box_floor(box_max[a], m.inv_leaf) : MAP_BIAS;
  }
  return sel;
}

int map_crop(ndt_handle* h, const float* box_min, const float* box_max, int remove_inside, int64_t* n_removed) {
  VoxelMap& m = *h->map;
  const MapSel sel = sel_box(m, box_min, box_max);
  size_t inside = 0;
  int rc = map_export_count(h, m, sel, true, &inside);   // (settles nvox_stale first; one host wait)
  if (rc) return rc;
  unsigned long long pts_inside = 0;
  if (m.n_voxels > 0) std::memcpy(&pts_inside, m.tsel_h.h + TS_POINTS, sizeof(pts_inside));
  else inside = 0;
  const int64_t kept = remove_inside ? m.n_voxels - (int64_t)inside : (int64_t)inside;
  const int64_t removed = m.n_voxels - kept;
  if (n_removed) *n_removed = removed;
  if (removed == 0) return NDT_OK;   // the table is as it was

  const int64_t new_cap = std::max(map_pow2_at_least(2 * kept), m.reset_capacity);
  rc = map_replace_table(h, m, new_cap, "voxel map crop: ", [&](const MapTable& fresh) {
    hipLaunchKernelGGL(k_mapstate_crop, dim3((unsigned)((m.tab.capacity + MAP_THREADS - 1) / MAP_THREADS)), dim3(MAP_THREADS), 0,
                       h->stream, m.tab, sel, remove_inside, fresh, m.stats.p, m.tsel.p);
    return NDT_OK;
  }, kept);
  if (rc) return rc;
  m.n_points = remove_inside ? m.n_points - (int64_t)pts_inside : (int64_t)pts_inside;
  return NDT_OK;
}

}  // namespace

// the selection's records, the first min(total, cap) of them, into device arrays (any may be null); *n_out = total
int map_export_state(ndt_handle* h, VoxelMap& m, const float* box_min, const float* box_max, int32_t* d_ijk, int32_t* d_count,
                     float* d_sums, double* d_mom, size_t cap, size_t* total_out) {
  const MapSel sel = sel_box(m, box_min, box_max);
  size_t total = 0;
  int rc = map_export_count(h, m, sel, true, &total);
  if (rc) return rc;
  *total_out = total;
  const size_t w = std::min(total, cap);
  if (w == 0 || !(d_ijk || d_count || d_sums || d_mom)) return NDT_OK;
  if (total >= (size_t)std::numeric_limits<int>::max()) return fail(h, NDT_ERR_INVALID_ARG, "too many voxels for one export");
  const int* ts = m.tsel_h.h;
  const int mn[3] = {ts[TS_MIN], ts[TS_MIN + 1], ts[TS_MIN + 2]}, mx[3] = {ts[TS_MAX], ts[TS_MAX + 1], ts[TS_MAX + 2]};
  const uint32_t *order = nullptr, *slots = nullptr;
  rc = map_export_order(h, m, sel, true, total, mn, mx, &order, &slots);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mapstate_gather, dim3((unsigned)((w + MAP_THREADS - 1) / MAP_THREADS)), dim3(MAP_THREADS), 0, h->stream, order,
                     slots, (int)w, m.tab.keys, m.tab.sums, m.tab.cnt, m.tab.mom, d_ijk, d_count, d_sums, d_mom);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NDT_OK;
}

// The n records' keys (m.pkey), grouped by their slot in table `t` (map_group_batch; *d_nvox goes up by the voxels they
// create there), continue the sums `t` holds: per voxel its records in input order, old + record.field.  After
// group_scratch(n, n + 1); enqueued, not awaited.
int map_merge_records(ndt_handle* h, const MapTable& t, unsigned long long* d_nvox, const int32_t* d_count, const float* d_sums,
                      const double* d_mom, size_t n) {
  VoxelMap& m = *h->map;
  hipStream_t s = h->stream;
  const unsigned blocks = (unsigned)((n + MAP_THREADS - 1) / MAP_THREADS);
  const uint32_t *keys_sorted = nullptr, *vals_sorted = nullptr;
  const int rc = map_group_batch(h, m, n, t, d_nvox, &keys_sorted, &vals_sorted);
  if (rc) return rc;
  if (m.moments)
    hipLaunchKernelGGL(k_mapstate_accumulate<true>, dim3(blocks), dim3(MAP_THREADS), 0, s, h->nleaf.p, h->leaf_start.p, h->leaf_cnt.p,
                       keys_sorted, vals_sorted, d_count, d_sums, d_mom, m.with_intensity, t.sums, t.cnt, t.mom);
  else
    hipLaunchKernelGGL(k_mapstate_accumulate<false>, dim3(blocks), dim3(MAP_THREADS), 0, s, h->nleaf.p, h->leaf_start.p, h->leaf_cnt.p,
                       keys_sorted, vals_sorted, d_count, d_sums, static_cast<const double*>(nullptr), m.with_intensity,
                       t.sums, t.cnt, static_cast<double*>(nullptr));
  HIP_TRY(h, hipGetLastError());
  return NDT_OK;
}

// The import behind its key pass (k_mapstate_keys, or the re-pose's record pass: m.pkey and m.stats are enqueued on the
// stream): the one host wait, the refusals, the growth, the counters and the merge of the n records; awaited.
int map_import_tail(ndt_handle* h, const int32_t* d_count, const float* d_sums, const double* d_mom, size_t n) {
  VoxelMap& m = *h->map;
  hipStream_t s = h->stream;
  int rc = NDT_OK;
  HIP_TRY(h, hipMemcpyAsync(m.stats_h.h, m.stats.p, MS_WORDS * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(m.nvox_h.h, m.nvox.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));   // the import's one host wait: refusals and growth decision
  m.n_voxels = (int64_t)m.nvox_h.h[0];
  m.nvox_stale = false;
  const int* st = m.stats_h.h;
  if (st[MS_BAD_COUNT] > 0)
    return fail(h, NDT_ERR_INVALID_ARG, std::to_string(st[MS_BAD_COUNT]) + " record(s) with count < 1; nothing was imported");
  if (st[MS_OOR] > 0)
    return fail(h, NDT_ERR_GRID_OVERFLOW, std::to_string(st[MS_OOR]) + " record(s) beyond the map's coordinate range (|voxel index| < 2^20 per axis); nothing was imported");
  const int64_t want = map_pow2_at_least(2 * (m.n_voxels + (int64_t)n));
  if (want > m.tab.capacity) {
    if (want > MAP_MAX_CAPACITY) return fail(h, NDT_ERR_ALLOC, "voxel map: more than 2^30 table slots needed");
    rc = map_grow_table(h, m, want);
    if (rc) return rc;
  }
  // from here on the map changes
  ++m.change;
  unsigned long long pts = 0;
  std::memcpy(&pts, st + MS_POINTS, sizeof(pts));
  ++m.n_adds;
  for (int a = 0; a < 3; ++a) {
    m.mn[a] = m.n_points ? std::min(m.mn[a], st[MS_MIN + a]) : st[MS_MIN + a];
    m.mx[a] = m.n_points ? std::max(m.mx[a], st[MS_MAX + a]) : st[MS_MAX + a];
  }
  m.n_points += (int64_t)pts;
  m.nvox_stale = true;
  rc = map_merge_records(h, m.tab, m.nvox.p, d_count, d_sums, d_mom, n);
  if (rc) return rc;
  // the caller's arrays (and the engine's scratch) are free again when the call returns
  HIP_TRY(h, hipStreamSynchronize(s));
  return NDT_OK;
}

namespace {

// n records in device memory (d_mom may be null in a map without moments), behind the argument checks
int map_import_state(ndt_handle* h, const int32_t* d_ijk, const int32_t* d_count, const float* d_sums, const double* d_mom, size_t n) {
  VoxelMap& m = *h->map;
  hipStream_t s = h->stream;
  // every allocation of the import except the table's growth, before anything is written
  HIP_TRY(h, m.pkey.ensure(n));
  const int rc = group_scratch(h, n, n + 1);
  if (rc) return rc;
  const unsigned blocks = (unsigned)((n + MAP_THREADS - 1) / MAP_THREADS);
  HIP_TRY(h, hipMemcpyAsync(m.stats.p, m.stats_h.h + MS_WORDS, MS_WORDS * sizeof(int), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_mapstate_keys, dim3(blocks), dim3(MAP_THREADS), 0, s, d_ijk, d_count, (int)n, m.pkey.p, m.stats.p);
  HIP_TRY(h, hipGetLastError());
  return map_import_tail(h, d_count, d_sums, d_mom, n);
}

}  // namespace

// what every import form checks once the map is known; *go: there is something to import
int map_import_checks(ndt_handle* h, float leaf, const double* moments9, size_t n, bool* go) {
  *go = false;
  if (!h->map) return no_map(h);
  VoxelMap& m = *h->map;
  if (std::memcmp(&m.leaf, &leaf, sizeof(float)) != 0)
    return fail(h, NDT_ERR_INVALID_ARG, "the state's leaf size is not the map's: a voxel of one is not a voxel of the other");
  if (m.moments && !moments9 && n) return fail(h, NDT_ERR_INVALID_ARG, "the map keeps moments: every import must bring them");
  if (n > (size_t)std::numeric_limits<int>::max() / 2) return fail(h, NDT_ERR_INVALID_ARG, "too many records");
  *go = n > 0;
  return NDT_OK;
}

// Both public forms of the state export on `m` -- the map or one of its levels -- behind the handle checks: the
// refusals, then the records into the caller's device arrays (device_out) or through m's staging arrays to the host.
int map_export_state_public(ndt_handle* h, VoxelMap& m, bool device_out, const float* box_min, const float* box_max, int32_t* ijk,
                            int32_t* count, float* sums4, double* moments9, size_t cap, size_t* n_out) {
  if (moments9 && !m.moments) return no_moments(h);
  if (box_min && !(finite3(box_min) && finite3(box_max))) return fail(h, NDT_ERR_INVALID_ARG, "non-finite box");
  settle_discard_keep_grid(h);
  int rc = NDT_OK;
  size_t total = 0;
  if (device_out) {
    rc = map_export_state(h, m, box_min, box_max, ijk, count, sums4, moments9, cap, &total);
    if (rc) return rc;
    *n_out = total;
  } else {
    rc = map_refresh_voxel_count(h, m);
    if (rc) return rc;
    // (no selection holds more than the map: the device-side outputs are sized before the selection is counted)
    const size_t w = std::min((size_t)m.n_voxels, cap);
    if (w) {
      if (ijk) HIP_TRY(h, m.xijk.ensure(3 * w));
      if (count) HIP_TRY(h, m.xcnt.ensure(w));
      if (sums4) HIP_TRY(h, m.xout.ensure(4 * w));
      if (moments9) HIP_TRY(h, m.xmom.ensure(9 * w));
    }
    rc = map_export_state(h, m, box_min, box_max, ijk && w ? m.xijk.p : nullptr, count && w ? m.xcnt.p : nullptr,
                          sums4 && w ? m.xout.p : nullptr, moments9 && w ? m.xmom.p : nullptr, w, &total);
    if (rc) return rc;
    *n_out = total;
    const size_t got = std::min(total, w);
    if (got) {
      if (ijk) HIP_TRY(h, hipMemcpy(ijk, m.xijk.p, 3 * got * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (count) HIP_TRY(h, hipMemcpy(count, m.xcnt.p, got * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (sums4) HIP_TRY(h, hipMemcpy(sums4, m.xout.p, 4 * got * sizeof(float), hipMemcpyDeviceToHost));
      if (moments9) HIP_TRY(h, hipMemcpy(moments9, m.xmom.p, 9 * got * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  if (total > cap) return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(total) + " voxels");
  return NDT_OK;
}

}  // namespace engine
}  // namespace ndt

extern "C" {

int ndt_map_crop(ndt_handle* h, const float box_min[3], const float box_max[3], int remove_inside, int64_t* n_removed) {
  if (!h || !box_min || !box_max) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  if (!(finite3(box_min) && finite3(box_max))) return fail(h, NDT_ERR_INVALID_ARG, "non-finite box");
  return map_crop(h, box_min, box_max, remove_inside, n_removed);
}

int ndt_map_export_state_device(ndt_handle* h, const float box_min[3], const float box_max[3], int32_t* ijk, int32_t* count,
                                float* sums4, double* moments9, size_t cap, size_t* n_out) {
  if (!h || !n_out || (box_min == nullptr) != (box_max == nullptr)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  return map_export_state_public(h, *h->map, true, box_min, box_max, ijk, count, sums4, moments9, cap, n_out);
}

int ndt_map_export_state(ndt_handle* h, const float box_min[3], const float box_max[3], int32_t* ijk, int32_t* count, float* sums4,
                         double* moments9, size_t cap, size_t* n_out) {
  if (!h || !n_out || (box_min == nullptr) != (box_max == nullptr)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  return map_export_state_public(h, *h->map, false, box_min, box_max, ijk, count, sums4, moments9, cap, n_out);
}

int ndt_map_import_state_device(ndt_handle* h, float leaf, const int32_t* ijk, const int32_t* count, const float* sums4,
                                const double* moments9, size_t n) {
  if (!h || ((!ijk || !count || !sums4) && n)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  bool go = false;
  rc = map_import_checks(h, leaf, moments9, n, &go);
  if (rc || !go) return rc;
  settle_discard_keep_grid(h);
  return map_import_state(h, ijk, count, sums4, h->map->moments ? moments9 : nullptr, n);
}

int ndt_map_import_state(ndt_handle* h, float leaf, const int32_t* ijk, const int32_t* count, const float* sums4,
                         const double* moments9, size_t n) {
  if (!h || ((!ijk || !count || !sums4) && n)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  bool go = false;
  rc = map_import_checks(h, leaf, moments9, n, &go);
  if (rc || !go) return rc;
  VoxelMap& m = *h->map;
  settle_discard_keep_grid(h);
  // the records on the device, in the host export's staging arrays
  HIP_TRY(h, m.xijk.ensure(3 * n));
  HIP_TRY(h, m.xcnt.ensure(n));
  HIP_TRY(h, m.xout.ensure(4 * n));
  if (m.moments) HIP_TRY(h, m.xmom.ensure(9 * n));
  HIP_TRY(h, hipMemcpy(m.xijk.p, ijk, 3 * n * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(m.xcnt.p, count, n * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(m.xout.p, sums4, 4 * n * sizeof(float), hipMemcpyHostToDevice));
  if (m.moments) HIP_TRY(h, hipMemcpy(m.xmom.p, moments9, 9 * n * sizeof(double), hipMemcpyHostToDevice));
  return map_import_state(h, m.xijk.p, m.xcnt.p, m.xout.p, m.moments ? m.xmom.p : nullptr, n);
}

}  // extern "C"
