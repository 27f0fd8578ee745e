// ndt_map_repose.hip -- the voxel map under a changed pose (see ndt_engine.h: VoxelMap; the rule: include/ndt_hip.h,
// ndt_map_transform): a voxel's record -- count, the four float sums, the nine f64 sums -- is moved by an affine map as
// the sums of its points would be, and goes to the voxel its moved float centroid falls into.
//   transform  the state export's gather into the staging arrays (ascending (k, j, i): the result does not depend on the
//              table's slot layout) -> k_maprepose_records in place (ONE host wait behind it: a voxel that would leave the
//              coordinate range refuses the whole call) -> the import's merge into a FRESH table, which replaces the map's
//              once it stands (map_grow_table with a refill -> map_replace_table)
//   import     k_maprepose_records from the caller's records into the staging arrays -> the import's own tail
//              (map_import_tail: the one host wait, refusals, growth, counters, merge)
// k_maprepose_records is the import's key pass (k_mapstate_keys) with the key taken from the moved centroid: the same
// statistics (map_record_stats), one integer atomic per word and block; wave64; no kernel waits for another block.  Every
// f64 operation rounds as written (-ffp-contract=off), so an elementwise restatement reproduces the records bit for bit.
#include "ndt_engine.h"
#include "ndt_map_device.h"

namespace ndt {

namespace {

// the upper 3 x 4 of the pose as given: R[3 * a + b] = R_ab, t[a]
struct ReposeConsts {
  double R[9];
  double t[3];
  float inv_leaf;
};

// (R_a0 * v0 + R_a1 * v1) + R_a2 * v2
__device__ __forceinline__ double repose_lin(const double* __restrict__ R, int a, double v0, double v1, double v2) {
  return (R[3 * a + 0] * v0 + R[3 * a + 1] * v1) + R[3 * a + 2] * v2;
}

// Record i (count, sums_in[4 i ..], MOM: mom_in[9 i ..]) moved by the pose -> sums_out / mom_out (which may be the
// inputs: a thread reads its whole record before it writes) and pkey[i], the key of the voxel the moved float centroid
// s' / (float)count falls into by the add's arithmetic (floor(c * inv_leaf) in f32).  MAP_EMPTY for count < 1 and for a
// centroid that is not finite or outside the coordinate range (both counted: the host refuses the whole call).  One
// thread per record: a wave reads 64 consecutive records, 4.6 KB of moments in nine loads 72 bytes apart per lane.
template <bool MOM>
__global__ void __launch_bounds__(MAP_THREADS) k_maprepose_records(const int32_t* __restrict__ count, const float* sums_in,
                                                                  const double* mom_in, int n, ReposeConsts pc, float* sums_out,
                                                                  double* mom_out, unsigned long long* __restrict__ pkey,
                                                                  int* __restrict__ stats) {
  const int i = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  int oor = 0, bad = 0;
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  unsigned long long pts = 0;
  if (i < n) {
    const int c = count[i];
    unsigned long long key = MAP_EMPTY;
    if (c < 1) {
      bad = 1;
    } else {
      const double* R = pc.R;
      const double* t = pc.t;
      const double nd = (double)c;
      const double nt[3] = {nd * t[0], nd * t[1], nd * t[2]};
      const float s0 = sums_in[(size_t)i * 4 + 0], s1 = sums_in[(size_t)i * 4 + 1], s2 = sums_in[(size_t)i * 4 + 2],
                  s3 = sums_in[(size_t)i * 4 + 3];
      double q[9];
      if (MOM) {
#pragma unroll
        for (int a = 0; a < 9; ++a) q[a] = mom_in[(size_t)i * 9 + a];
      }
      float sp[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) sp[a] = (float)(repose_lin(R, a, (double)s0, (double)s1, (double)s2) + nt[a]);
      sums_out[(size_t)i * 4 + 0] = sp[0]; sums_out[(size_t)i * 4 + 1] = sp[1]; sums_out[(size_t)i * 4 + 2] = sp[2];
      sums_out[(size_t)i * 4 + 3] = s3;
      if (MOM) {
        double u[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) u[a] = repose_lin(R, a, q[0], q[1], q[2]);
        const double M[3][3] = {{q[3], q[4], q[5]}, {q[4], q[6], q[7]}, {q[5], q[7], q[8]}};
        double A[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) A[a][b] = repose_lin(R, a, M[0][b], M[1][b], M[2][b]);
        double o[9];
        int w = 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          o[a] = u[a] + nt[a];
#pragma unroll
          for (int b = a; b < 3; ++b) {
            const double B = (A[a][0] * R[3 * b + 0] + A[a][1] * R[3 * b + 1]) + A[a][2] * R[3 * b + 2];
            o[w++] = ((B + u[a] * t[b]) + t[a] * u[b]) + nt[a] * t[b];
          }
        }
#pragma unroll
        for (int a = 0; a < 9; ++a) mom_out[(size_t)i * 9 + a] = o[a];
      }
      const float nf = (float)c;
      const float cx = sp[0] / nf, cy = sp[1] / nf, cz = sp[2] / nf;
      bool in_range = false;
      if (isfinite(cx) && isfinite(cy) && isfinite(cz)) {
        const float fi = floorf(cx * pc.inv_leaf), fj = floorf(cy * pc.inv_leaf), fk = floorf(cz * pc.inv_leaf);
        if (fabsf(fi) < MAP_LIMIT && fabsf(fj) < MAP_LIMIT && fabsf(fk) < MAP_LIMIT) {
          const int vi = (int)fi, vj = (int)fj, vk = (int)fk;
          in_range = true;
          mn[0] = mx[0] = vi; mn[1] = mx[1] = vj; mn[2] = mx[2] = vk;
          pts = (unsigned long long)c;
          key = map_key(vi, vj, vk);
        }
      }
      if (!in_range) oor = 1;
    }
    pkey[i] = key;
  }
  map_record_stats(oor, bad, pts, mn, mx, stats);
}

}  // namespace

namespace engine {
namespace {

// the record pass over n records on the engine's stream, its statistics starting from the neutral words; enqueued
int repose_records(ndt_handle* h, const double* pose16, const int32_t* d_count, const float* sums_in, const double* mom_in, size_t n,
                   float* sums_out, double* mom_out) {
  VoxelMap& m = *h->map;
  hipStream_t s = h->stream;
  ReposeConsts pc;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) pc.R[3 * a + b] = pose16[a + 4 * b];
    pc.t[a] = pose16[12 + a];
  }
  pc.inv_leaf = m.inv_leaf;
  const unsigned blocks = (unsigned)((n + MAP_THREADS - 1) / MAP_THREADS);
  HIP_TRY(h, hipMemcpyAsync(m.stats.p, m.stats_h.h + MS_WORDS, MS_WORDS * sizeof(int), hipMemcpyHostToDevice, s));
  if (m.moments)
    hipLaunchKernelGGL(k_maprepose_records<true>, dim3(blocks), dim3(MAP_THREADS), 0, s, d_count, sums_in, mom_in, (int)n, pc, sums_out,
                       mom_out, m.pkey.p, m.stats.p);
  else
    hipLaunchKernelGGL(k_maprepose_records<false>, dim3(blocks), dim3(MAP_THREADS), 0, s, d_count, sums_in,
                       static_cast<const double*>(nullptr), (int)n, pc, sums_out, static_cast<double*>(nullptr), m.pkey.p, m.stats.p);
  HIP_TRY(h, hipGetLastError());
  return NDT_OK;
}

// ndt_map_transform behind its argument checks
int map_transform(ndt_handle* h, const double* pose16, int64_t* n_after) {
  VoxelMap& m = *h->map;
  hipStream_t s = h->stream;
  int rc = map_refresh_voxel_count(h, m);
  if (rc) return rc;
  if (m.n_voxels == 0) {   // untouched
    if (n_after) *n_after = 0;
    return NDT_OK;
  }
  const size_t n = (size_t)m.n_voxels;
  if (n > (size_t)std::numeric_limits<int>::max() / 2) return fail(h, NDT_ERR_INVALID_ARG, "too many voxels for one transform");
  const int64_t new_cap = std::max(map_pow2_at_least(2 * (int64_t)n), m.reset_capacity);
  if (new_cap > MAP_MAX_CAPACITY) return fail(h, NDT_ERR_ALLOC, "voxel map: more than 2^30 table slots needed");
  // every allocation of the call except the fresh table, before anything is written
  HIP_TRY(h, m.xcnt.ensure(n));
  HIP_TRY(h, m.xout.ensure(4 * n));
  if (m.moments) HIP_TRY(h, m.xmom.ensure(9 * n));
  HIP_TRY(h, m.pkey.ensure(n));
  rc = group_scratch(h, n, n + 1);
  if (rc) return rc;
  // the records in export-state order, in the staging arrays
  size_t total = 0;
  rc = map_export_state(h, m, nullptr, nullptr, nullptr, m.xcnt.p, m.xout.p, m.moments ? m.xmom.p : nullptr, n, &total);
  if (rc) return rc;
  if (total != n) return fail(h, NDT_ERR_HIP, "voxel map transform: the table holds " + std::to_string(total) + " voxels, the counter says " + std::to_string(n));
  rc = repose_records(h, pose16, m.xcnt.p, m.xout.p, m.moments ? m.xmom.p : nullptr, n, m.xout.p, m.moments ? m.xmom.p : nullptr);
  if (rc) return rc;
  HIP_TRY(h, hipMemcpyAsync(m.stats_h.h, m.stats.p, MS_WORDS * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));   // the refusal is decided before anything of the map is written
  const int* st = m.stats_h.h;
  if (st[MS_OOR] > 0 || st[MS_BAD_COUNT] > 0)
    return fail(h, NDT_ERR_GRID_OVERFLOW, std::to_string(st[MS_OOR] + st[MS_BAD_COUNT]) + " voxel(s) would move beyond the map's coordinate range (|voxel index| < 2^20 per axis) or to a non-finite place; the map is as it was");
  const int mn[3] = {st[MS_MIN], st[MS_MIN + 1], st[MS_MIN + 2]}, mx[3] = {st[MS_MAX], st[MS_MAX + 1], st[MS_MAX + 2]};
  const MapRefill refill{"voxel map transform: ", [&](const MapTable& fresh) {
    return map_merge_records(h, fresh, m.nvox.p + 1, m.xcnt.p, m.xout.p, m.moments ? m.xmom.p : nullptr, n);
  }};
  rc = map_grow_table(h, m, new_cap, &refill);
  if (rc) return rc;
  for (int a = 0; a < 3; ++a) { m.mn[a] = mn[a]; m.mx[a] = mx[a]; }
  if (n_after) *n_after = m.n_voxels;
  return NDT_OK;
}

// both posed import forms behind their checks: the caller's records (device memory) moved into the staging arrays, then
// the import's tail
int map_import_posed(ndt_handle* h, const double* pose16, const int32_t* d_count, const float* d_sums, const double* d_mom, size_t n) {
  VoxelMap& m = *h->map;
  // every allocation of the import except the table's growth, before anything is written
  HIP_TRY(h, m.xout.ensure(4 * n));
  if (m.moments) HIP_TRY(h, m.xmom.ensure(9 * n));
  HIP_TRY(h, m.pkey.ensure(n));
  int rc = group_scratch(h, n, n + 1);
  if (rc) return rc;
  rc = repose_records(h, pose16, d_count, d_sums, m.moments ? d_mom : nullptr, n, m.xout.p, m.moments ? m.xmom.p : nullptr);
  if (rc) return rc;
  return map_import_tail(h, d_count, m.xout.p, m.moments ? m.xmom.p : nullptr, n);
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

int ndt_map_transform(ndt_handle* h, const double pose16_colmajor[16], int64_t* n_voxels_after_or_null) {
  if (!h || !pose16_colmajor) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  if (!pose_finite(pose16_colmajor)) return fail(h, NDT_ERR_INVALID_ARG, "non-finite pose");
  settle_discard_keep_grid(h);
  return map_transform(h, pose16_colmajor, n_voxels_after_or_null);
}

int ndt_map_import_state_posed_device(ndt_handle* h, float leaf, const int32_t* ijk, const int32_t* count, const float* sums4,
                                      const double* moments9, size_t n, const double pose16_colmajor[16]) {
  if (!h || !pose16_colmajor || ((!ijk || !count || !sums4) && n)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  bool go = false;
  rc = map_import_checks(h, leaf, moments9, n, &go);
  if (rc) return rc;
  if (!pose_finite(pose16_colmajor)) return fail(h, NDT_ERR_INVALID_ARG, "non-finite pose");
  if (!go) return NDT_OK;
  settle_discard_keep_grid(h);
  return map_import_posed(h, pose16_colmajor, count, sums4, moments9, n);
}

int ndt_map_import_state_posed(ndt_handle* h, float leaf, const int32_t* ijk, const int32_t* count, const float* sums4,
                               const double* moments9, size_t n, const double pose16_colmajor[16]) {
  if (!h || !pose16_colmajor || ((!ijk || !count || !sums4) && n)) return NDT_ERR_INVALID_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  bool go = false;
  rc = map_import_checks(h, leaf, moments9, n, &go);
  if (rc) return rc;
  if (!pose_finite(pose16_colmajor)) return fail(h, NDT_ERR_INVALID_ARG, "non-finite pose");
  if (!go) return NDT_OK;
  VoxelMap& m = *h->map;
  settle_discard_keep_grid(h);
  // the records on the device, in the host export's staging arrays (the rule does not read ijk: the moved centroid decides)
  HIP_TRY(h, m.xcnt.ensure(n));
  HIP_TRY(h, m.xout.ensure(4 * n));
  if (m.moments) HIP_TRY(h, m.xmom.ensure(9 * n));
  HIP_TRY(h, hipMemcpy(m.xcnt.p, count, n * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(m.xout.p, sums4, 4 * n * sizeof(float), hipMemcpyHostToDevice));
  if (m.moments) HIP_TRY(h, hipMemcpy(m.xmom.p, moments9, 9 * n * sizeof(double), hipMemcpyHostToDevice));
  return map_import_posed(h, pose16_colmajor, m.xcnt.p, m.xout.p, m.moments ? m.xmom.p : nullptr, n);
}

}  // extern "C"
