// ndt_map_carve.hip -- free-space carving of the voxel map (ndt_map_carve*, see ndt_engine.h: VoxelMap): a measured ray
// from the sensor to a return says that every voxel it crosses before the return is empty now, so a voxel that enough
// rays of one scan pass through, and none ends in, leaves the map (NDT-OM's answer to the trails of what moved).
//   rays     one thread per ray: [transform] -> start / end voxel -> Amanatides-Woo in f64, in voxel units, every
//            operation rounded as written -> a read-only probe of the table per voxel of the path (map_find) -> one
//            integer atomic on the slot's mark word: +1 for a miss, the top bit for the hit at the ray's end
//   count    one pass over the slots: voxels crossed, voxels hit, voxels to remove and their points (ONE host wait: the
//            result is known, and whether anything moves and how large the new table is)
//   move     the crop's move under the mark predicate: the survivors go to a fresh table as they are, the same launch
//            reducing their tight ijk box
// The marks are sums and ORs of integers: whatever the order of the rays, the words are the same.  They are scratch of
// the call; the table's persistent state is untouched until the move.
// The rules of ndt_map.hip hold: wave64, integer atomics only, no kernel waits for another block, every loop is bounded
// (the walk by max_steps, a probe by the capacity).
#include "ndt_engine.h"
#include "ndt_map_device.h"

namespace ndt {

namespace {

constexpr unsigned int CARVE_HIT = 0x80000000u;   // a mark word: misses in the low 31 bits (a ray crosses a voxel once, n < 2^30)
constexpr double CARVE_LIMIT = 1048576.0;         // MAP_LIMIT in f64
// words of VoxelMap::cstat
enum { CS_SKIPPED = 0, CS_STEPS = 1, CS_CROSSED = 2, CS_HIT = 3, CS_REMOVED = 4, CS_POINTS = 5, CS_WORDS = 8 };

// What one launch of k_mapcarve_rays knows about its call: the pose as ndt_map_add applies it, the origin behind the pose
// in voxel units and its voxel, the limits.
struct CarveRays {
  double R[9], t[3];      // row-major rotation and translation (has_pose)
  double gs[3];           // (double)(origin_f32 * inv_leaf_f32) per axis
  int vs[3];              // floor(gs)
  int has_pose;
  int origin_in_range;    // |vs| < 2^20 on every axis; otherwise every ray is skipped
  float inv_leaf;
  int keep_last, max_steps;
};

// Ray i runs from the origin to point i.  Path v_0 = vs .. v_L = ve, L = |ve - vs|_1: every step advances the axis with
// the smallest tMax (the lowest axis on equal values), an axis that has reached ve[a] has tMax = +inf.  v_i takes a miss
// for 1 <= i <= min(L - 1 - keep_last, max_steps), v_L the hit; only voxels the table holds take marks.  The three axes
// are kept in named scalars (no runtime-indexed arrays: they would live in scratch).
__global__ void __launch_bounds__(MAP_THREADS) k_mapcarve_rays(const float* __restrict__ x, const float* __restrict__ y,
                                                              const float* __restrict__ z, int n, CarveRays c,
                                                              const unsigned long long* __restrict__ tkeys,
                                                              unsigned long long mask, unsigned int* __restrict__ marks,
                                                              unsigned long long* __restrict__ cstat) {
  __shared__ unsigned long long red[MAP_WAVES][2];
  const int i = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  unsigned long long skipped = 0, steps = 0;
  if (i < n) {
    float a = x[i], b = y[i], d = z[i];
    bool ok = isfinite(a) && isfinite(b) && isfinite(d);
    if (ok && c.has_pose) {
      const double pa = (double)a, pb = (double)b, pc = (double)d;
      a = (float)(c.R[0] * pa + c.R[1] * pb + c.R[2] * pc + c.t[0]);
      b = (float)(c.R[3] * pa + c.R[4] * pb + c.R[5] * pc + c.t[1]);
      d = (float)(c.R[6] * pa + c.R[7] * pb + c.R[8] * pc + c.t[2]);
      ok = isfinite(a) && isfinite(b) && isfinite(d);
    }
    const double gx = (double)(a * c.inv_leaf), gy = (double)(b * c.inv_leaf), gz = (double)(d * c.inv_leaf);
    const double fx = floor(gx), fy = floor(gy), fz = floor(gz);
    ok = ok && c.origin_in_range != 0 && fabs(fx) < CARVE_LIMIT && fabs(fy) < CARVE_LIMIT && fabs(fz) < CARVE_LIMIT;
    if (!ok) {
      skipped = 1;
    } else {
      const int ex = (int)fx, ey = (int)fy, ez = (int)fz;
      int vx = c.vs[0], vy = c.vs[1], vz = c.vs[2];
      const long long L = (long long)abs(ex - vx) + (long long)abs(ey - vy) + (long long)abs(ez - vz);
      long long bound = L - 1 - (long long)c.keep_last;
      if (bound > (long long)c.max_steps) bound = (long long)c.max_steps;
      if (bound < 0) bound = 0;
      steps = (unsigned long long)bound;
      const double inf = __longlong_as_double(0x7ff0000000000000ll);
      const double dx = gx - c.gs[0], dy = gy - c.gs[1], dz = gz - c.gs[2];
      const int sx = ex > vx ? 1 : -1, sy = ey > vy ? 1 : -1, sz = ez > vz ? 1 : -1;
      double tdx = 0.0, tdy = 0.0, tdz = 0.0, tx = inf, ty = inf, tz = inf;
      if (ex != vx) { tdx = 1.0 / fabs(dx); tx = ((double)(vx + (sx > 0 ? 1 : 0)) - c.gs[0]) / dx; }
      if (ey != vy) { tdy = 1.0 / fabs(dy); ty = ((double)(vy + (sy > 0 ? 1 : 0)) - c.gs[1]) / dy; }
      if (ez != vz) { tdz = 1.0 / fabs(dz); tz = ((double)(vz + (sz > 0 ? 1 : 0)) - c.gs[2]) / dz; }
      for (long long k = 0; k < bound; ++k) {   // (bound <= max_steps <= 65536)
        if (tx <= ty && tx <= tz) { vx += sx; tx = vx == ex ? inf : tx + tdx; }
        else if (ty <= tz) { vy += sy; ty = vy == ey ? inf : ty + tdy; }
        else { vz += sz; tz = vz == ez ? inf : tz + tdz; }
        const long long s = map_find(tkeys, mask, map_key(vx, vy, vz));
        if (s >= 0) atomicAdd(marks + s, 1u);
      }
      const long long s = map_find(tkeys, mask, map_key(ex, ey, ez));
      if (s >= 0) atomicOr(marks + s, CARVE_HIT);
    }
  }
  skipped = wave_sum_u64(skipped);
  steps = wave_sum_u64(steps);
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  if (lane == 0) { red[wave][0] = skipped; red[wave][1] = steps; }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) v += red[w][threadIdx.x];
    if (v) atomicAdd(cstat + (threadIdx.x == 0 ? CS_SKIPPED : CS_STEPS), v);
  }
}

// what goes: enough misses, no hit, and not protected by its count
__device__ __forceinline__ bool carve_removes(unsigned int mark, int count, int min_misses, int protect_min_count) {
  return (mark & CARVE_HIT) == 0u && mark >= (unsigned int)min_misses && (protect_min_count == 0 || count < protect_min_count);
}

// the occupied voxels with a miss, those with a hit, those that go and the points they hold: one integer atomic per word
// and block
__global__ void __launch_bounds__(MAP_THREADS) k_mapcarve_count(const unsigned long long* __restrict__ tkeys,
                                                               const int* __restrict__ cnt,
                                                               const unsigned int* __restrict__ marks, long long cap,
                                                               int min_misses, int protect_min_count,
                                                               unsigned long long* __restrict__ cstat) {
  __shared__ unsigned long long red[MAP_WAVES][4];
  const long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
  unsigned long long crossed = 0, hit = 0, removed = 0, pts = 0;
  if (i < cap && tkeys[i] != MAP_EMPTY) {
    const unsigned int mark = marks[i];
    if (mark != 0u) {
      const int count = cnt[i];
      crossed = (mark & ~CARVE_HIT) != 0u ? 1 : 0;
      hit = (mark & CARVE_HIT) != 0u ? 1 : 0;
      if (carve_removes(mark, count, min_misses, protect_min_count)) { removed = 1; pts = (unsigned long long)count; }
    }
  }
  crossed = wave_sum_u64(crossed);
  hit = wave_sum_u64(hit);
  removed = wave_sum_u64(removed);
  pts = wave_sum_u64(pts);
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  if (lane == 0) { red[wave][0] = crossed; red[wave][1] = hit; red[wave][2] = removed; red[wave][3] = pts; }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) v += red[w][threadIdx.x];
    if (v) atomicAdd(cstat + CS_CROSSED + threadIdx.x, v);
  }
}

// Every occupied slot of the old table that stays moves to the new table (map_move_slot); the survivors' ijk box goes to
// tsel (TS_MIN / TS_MAX).  k_mapstate_crop under the mark predicate.
__global__ void __launch_bounds__(MAP_THREADS) k_mapcarve_move(MapTable o, const unsigned int* __restrict__ marks, int min_misses,
                                                              int protect_min_count, MapTable t, int* __restrict__ stats,
                                                              int* __restrict__ tsel) {
  __shared__ int box[MAP_WAVES][6];
  const long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  if (i < o.capacity) {
    const unsigned long long key = o.keys[i];
    if (key != MAP_EMPTY && !carve_removes(marks[i], o.cnt[i], min_misses, protect_min_count) &&
        map_move_slot(o, i, key, t, stats)) {
      map_ijk(key, mn);
      map_ijk(key, mx);
    }
  }
  map_box_waves(mn, mx, box);
  __syncthreads();
  map_box_commit(box, tsel + TS_MIN, tsel + TS_MAX);
}

}  // namespace

namespace engine {
namespace {

bool carve_params_valid(const ndt_map_carve_params* p) {
  return p->min_misses >= 1 && p->keep_last >= 0 && p->max_steps >= 1 && p->max_steps <= 65536 && p->protect_min_count >= 0 &&
         p->reserved[0] == 0 && p->reserved[1] == 0 && p->reserved[2] == 0;
}

// what every form refuses before the handle is looked at
bool carve_args_ok(const float* origin, const ndt_map_carve_params* prm) {
  return origin && prm && carve_params_valid(prm) && finite3(origin);
}

// One scan in device memory under an optional pose, behind the argument checks.
int map_carve_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n, const float* origin,
                     const double* pose16, const ndt_map_carve_params& prm, ndt_map_carve_result* out) {
  VoxelMap& m = *h->map;
  if (n == 0) {
    if (out) *out = ndt_map_carve_result{};
    return NDT_OK;
  }
  if (n > (size_t)std::numeric_limits<int>::max() / 2) return fail(h, NDT_ERR_INVALID_ARG, "cloud too large");
  CarveRays c{};
  c.has_pose = pose16 ? 1 : 0;
  c.inv_leaf = m.inv_leaf;
  c.keep_last = prm.keep_last;
  c.max_steps = prm.max_steps;
  float o[3] = {origin[0], origin[1], origin[2]};
  if (pose16) {   // (launch_transform_append's matrix and arithmetic)
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) c.R[3 * i + j] = pose16[4 * j + i];
      c.t[i] = pose16[12 + i];
    }
    const double a = (double)origin[0], b = (double)origin[1], d = (double)origin[2];
    for (int i = 0; i < 3; ++i) o[i] = (float)(c.R[3 * i] * a + c.R[3 * i + 1] * b + c.R[3 * i + 2] * d + c.t[i]);
    if (!finite3(o)) return fail(h, NDT_ERR_INVALID_ARG, "the origin is not finite behind the pose");
  }
  c.origin_in_range = 1;
  for (int a = 0; a < 3; ++a) {
    c.gs[a] = (double)(o[a] * m.inv_leaf);
    const double f = std::floor(c.gs[a]);
    if (std::fabs(f) < CARVE_LIMIT) c.vs[a] = (int)f;   // (an infinite product is out of range, not an error)
    else c.origin_in_range = 0;
  }
  settle_discard_keep_grid(h);
  hipStream_t s = h->stream;
  int rc = map_refresh_voxel_count(h, *h->map);
  if (rc) return rc;
  HIP_TRY(h, m.cmarks.ensure((size_t)m.tab.capacity));
  HIP_TRY(h, m.cstat.ensure(CS_WORDS));
  HIP_TRY(h, m.cstat_h.ensure(CS_WORDS));
  HIP_TRY(h, hipMemsetAsync(m.cmarks.p, 0, (size_t)m.tab.capacity * sizeof(unsigned int), s));
  HIP_TRY(h, hipMemsetAsync(m.cstat.p, 0, CS_WORDS * sizeof(unsigned long long), s));
  const unsigned ray_blocks = (unsigned)((n + MAP_THREADS - 1) / MAP_THREADS);
  const unsigned slot_blocks = (unsigned)((m.tab.capacity + MAP_THREADS - 1) / MAP_THREADS);
  hipLaunchKernelGGL(k_mapcarve_rays, dim3(ray_blocks), dim3(MAP_THREADS), 0, s, dx, dy, dz, (int)n, c, m.tab.keys,
                     (unsigned long long)(m.tab.capacity - 1), m.cmarks.p, m.cstat.p);
  HIP_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(k_mapcarve_count, dim3(slot_blocks), dim3(MAP_THREADS), 0, s, m.tab.keys, m.tab.cnt, m.cmarks.p, (long long)m.tab.capacity,
                     prm.min_misses, prm.protect_min_count, m.cstat.p);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(m.cstat_h.h, m.cstat.p, CS_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));   // the carve's one host wait: the result, and whether anything moves
  const unsigned long long* cs = m.cstat_h.h;
  const int64_t removed = (int64_t)cs[CS_REMOVED], pts_removed = (int64_t)cs[CS_POINTS];
  if (out) {
    *out = ndt_map_carve_result{};
    out->n_rays = (int64_t)n;
    out->n_rays_skipped = (int64_t)cs[CS_SKIPPED];
    out->n_steps = (int64_t)cs[CS_STEPS];
    out->n_voxels_crossed = (int64_t)cs[CS_CROSSED];
    out->n_voxels_hit = (int64_t)cs[CS_HIT];
    out->n_removed = removed;
    out->n_points_removed = pts_removed;
  }
  if (prm.dry_run || removed == 0) return NDT_OK;   // the table is as it was

  const int64_t kept = m.n_voxels - removed;
  const int64_t new_cap = std::max(map_pow2_at_least(2 * kept), m.reset_capacity);
  rc = map_replace_table(h, m, new_cap, "voxel map carve: ", [&](const MapTable& fresh) {
    hipLaunchKernelGGL(k_mapcarve_move, dim3(slot_blocks), dim3(MAP_THREADS), 0, s, m.tab, m.cmarks.p, prm.min_misses,
                       prm.protect_min_count, fresh, m.stats.p, m.tsel.p);
    return NDT_OK;
  }, kept);
  if (rc) return rc;
  m.n_points -= pts_removed;
  return NDT_OK;
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

void ndt_map_carve_default_params(ndt_map_carve_params* p) {
  if (!p) return;
  *p = ndt_map_carve_params{};
  p->min_misses = 2;
  p->keep_last = 1;
  p->max_steps = 4096;
}

int ndt_map_carve_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n, const float origin[3],
                         const double* pose16, const ndt_map_carve_params* prm, ndt_map_carve_result* out) {
  if (!h || ((!dx || !dy || !dz) && n) || !carve_args_ok(origin, prm)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  if (pose16 && !pose_finite(pose16)) return fail(h, NDT_ERR_INVALID_ARG, "non-finite pose");
  return map_carve_device(h, dx, dy, dz, n, origin, pose16, *prm, out);
}

int ndt_map_carve(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, const float origin[3], const double* pose16,
                  const ndt_map_carve_params* prm, ndt_map_carve_result* out) {
  if (!h || (!xyz && n) || !layout_valid(stride_bytes, -1) || !carve_args_ok(origin, prm)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  if (pose16 && !pose_finite(pose16)) return fail(h, NDT_ERR_INVALID_ARG, "non-finite pose");
  VoxelMap& m = *h->map;
  if (n == 0) return map_carve_device(h, nullptr, nullptr, nullptr, 0, origin, pose16, *prm, out);
  settle_discard_keep_grid(h);
  rc = upload_soa(h, h->lane_t, h->stream, xyz, nullptr, nullptr, nullptr, n, stride_bytes, m.ux, m.uy, m.uz, true);
  if (rc) return rc;
  return map_carve_device(h, m.ux.p, m.uy.p, m.uz.p, n, origin, pose16, *prm, out);
}

int ndt_map_carve_keyframe(ndt_handle* h, int64_t id, const float origin[3], const double pose16[16],
                           const ndt_map_carve_params* prm, ndt_map_carve_result* out) {
  if (!h || !pose16 || !carve_args_ok(origin, prm)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  if (!pose_finite(pose16)) return fail(h, NDT_ERR_INVALID_ARG, "non-finite pose");
  auto it = h->keyframes.find(id);
  if (it == h->keyframes.end()) return fail(h, NDT_ERR_INVALID_ARG, "unknown keyframe id");
  const ndt_handle::Keyframe& kf = it->second;
  return map_carve_device(h, kf.x.p, kf.y.p, kf.z.p, kf.n, origin, pose16, *prm, out);
}

}  // extern "C"
