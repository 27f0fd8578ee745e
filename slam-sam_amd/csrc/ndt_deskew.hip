// ndt_deskew.hip -- motion compensation of a scan from per-point times and a pose trajectory, with the acquisition
// filter of the drivers in the same pass (see ndt_trajectory.h for the model, include/ndt_hip.h for the contract).
//   aligned    (no filter)  ONE launch of k_deskew_aligned: out[i] = deskewed in[i], a non-finite point -> NaN
//   compacting (filter)     the stable compaction of ndt_compact_device.h in three launches: k_deskew_count, the
//                           one-block scan (launch_filter_scan), k_deskew_emit (the deskewed point behind its offset)
// One thread per point, coalesced SoA loads; the knot table (<= 64 rows of 12 doubles) is copied into LDS by every block
// and the segment is a binary search in it.  Integer offsets only, no atomics.  Everything on the engine's stream;
// the target, the source, the align state, the history and the counters of the handle are not touched.
// The predicate (dsk_keep), the knot table's LDS copy and the motion (dsk_move) live in ndt_deskew_device.h, shared with
// ndt_unproject.hip; the host's upload of the knot table is in this file, the strided download of a result with the
// rest of the host-cloud boundary (ndt_host_cloud.h, ndt_handoff.hip).
#include "ndt_engine.h"
#include "ndt_compact_device.h"
#include "ndt_deskew_device.h"
#include "ndt_trajectory.h"

namespace ndt {

namespace {

// (no __restrict__ on the clouds: the outputs may be the inputs -- every thread reads its point before it writes it)
__global__ void __launch_bounds__(DSK_THREADS) k_deskew_aligned(const float* sx, const float* sy, const float* sz, const float* st,
                                                               const float* si, unsigned int n, const double* __restrict__ table,
                                                               int n_knots, float* ox, float* oy, float* oz, float* oi,
                                                               int* o_index) {
  __shared__ double s_tab[traj::MAX_KNOTS * traj::ROW_WORDS];
  dsk_load_table(table, n_knots, s_tab);
  const unsigned int i = blockIdx.x * DSK_THREADS + threadIdx.x;
  if (i >= n) return;
  const float x = sx[i], y = sy[i], z = sz[i], t = st[i];
  float rx, ry, rz;
  if (isfinite(x) && isfinite(y) && isfinite(z) && isfinite(t)) {
    dsk_move(reinterpret_cast<const traj::KnotRow*>(s_tab), n_knots, x, y, z, t, &rx, &ry, &rz);
  } else {
    rx = ry = rz = __builtin_nanf("");
  }
  const float inten = oi ? si[i] : 0.0f;
  ox[i] = rx;
  oy[i] = ry;
  oz[i] = rz;
  if (oi) oi[i] = inten;
  if (o_index) o_index[i] = (int)i;
}

__global__ void __launch_bounds__(DSK_THREADS) k_deskew_count(const float* __restrict__ sx, const float* __restrict__ sy,
                                                             const float* __restrict__ sz, const float* __restrict__ st,
                                                             const float* __restrict__ si, unsigned int n, ndt_scan_filter f,
                                                             unsigned int* __restrict__ counts) {
  __shared__ unsigned int s_w[DSK_WAVES];
  const unsigned int i = blockIdx.x * DSK_THREADS + threadIdx.x;
  compact_ballot(i < n && dsk_keep(f, sx[i], sy[i], sz[i], st[i], si, i), s_w);
  __syncthreads();
  compact_block_count(s_w, counts);
}

__global__ void __launch_bounds__(DSK_THREADS) k_deskew_emit(const float* __restrict__ sx, const float* __restrict__ sy,
                                                            const float* __restrict__ sz, const float* __restrict__ st,
                                                            const float* __restrict__ si, unsigned int n, ndt_scan_filter f,
                                                            const double* __restrict__ table, int n_knots,
                                                            const unsigned int* __restrict__ offsets, float* __restrict__ ox,
                                                            float* __restrict__ oy, float* __restrict__ oz, float* __restrict__ oi,
                                                            int* __restrict__ o_index, unsigned int cap) {
  __shared__ double s_tab[traj::MAX_KNOTS * traj::ROW_WORDS];
  __shared__ unsigned int s_w[DSK_WAVES];
  const unsigned int i = blockIdx.x * DSK_THREADS + threadIdx.x;
  float x = 0.0f, y = 0.0f, z = 0.0f, t = 0.0f;
  bool keep = false;
  if (i < n) {
    x = sx[i]; y = sy[i]; z = sz[i]; t = st[i];
    keep = dsk_keep(f, x, y, z, t, si, i);
  }
  const unsigned long long bal = compact_ballot(keep, s_w);
  dsk_load_table(table, n_knots, s_tab);   // (its barrier also publishes s_w)
  const unsigned int pos = compact_position(bal, s_w, offsets);
  if (keep && pos < cap) {   // (the output holds cap points: a selection beyond it is counted, not written)
    float rx, ry, rz;
    dsk_move(reinterpret_cast<const traj::KnotRow*>(s_tab), n_knots, x, y, z, t, &rx, &ry, &rz);
    ox[pos] = rx;
    oy[pos] = ry;
    oz[pos] = rz;
    if (oi) oi[pos] = si[i];
    if (o_index) o_index[pos] = (int)i;
  }
}

}  // namespace

namespace engine {

int knots_upload(ndt_handle* h, const traj::KnotRow* rows, int n_knots) {
  KnotTable& k = h->knots;
  HIP_TRY(h, k.tab.ensure((size_t)traj::MAX_KNOTS * traj::ROW_WORDS));
  HIP_TRY(h, k.tab_h.ensure((size_t)traj::MAX_KNOTS * traj::ROW_WORDS));
  if (n_knots > 0) {
    const size_t tab_bytes = (size_t)n_knots * sizeof(traj::KnotRow);
    std::memcpy(k.tab_h.h, rows, tab_bytes);   // (the previous call's copy out of the staging has been awaited)
    HIP_TRY(h, hipMemcpyAsync(k.tab.p, k.tab_h.h, tab_bytes, hipMemcpyHostToDevice, h->stream));
  }
  return NDT_OK;
}

namespace {

// The trajectory's table to the device (knots_upload), then the launches; awaited.  dx .. dt (and di, ox .. o_index) are
// device arrays.  Arguments have been checked.
int deskew_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, const float* di, const float* dt, size_t n,
                  const traj::KnotRow* rows, int n_knots, const ndt_scan_filter* filter, float* ox, float* oy, float* oz, float* oi,
                  int32_t* o_index, size_t cap, size_t* n_out) {
  *n_out = 0;
  if (n == 0) return NDT_OK;
  hipStream_t s = h->stream;
  int rc = knots_upload(h, rows, n_knots);
  if (rc) return rc;
  const double* tab = h->knots.tab.p;
  const int nb = (int)((n + DSK_THREADS - 1) / DSK_THREADS);
  static_assert(sizeof(int) == sizeof(int32_t), "index type");
  if (!filter) {
    hipLaunchKernelGGL(k_deskew_aligned, dim3((unsigned)nb), dim3(DSK_THREADS), 0, s, dx, dy, dz, dt, di, (unsigned int)n, tab,
                       n_knots, ox, oy, oz, di ? oi : nullptr, o_index);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));
    *n_out = n;
    return NDT_OK;
  }
  rc = compact_scratch(h, nb);
  if (rc) return rc;
  unsigned int* counts = h->compact.counts.p;
  const unsigned int ucap = (unsigned int)std::min<size_t>(cap, n);
  hipLaunchKernelGGL(k_deskew_count, dim3((unsigned)nb), dim3(DSK_THREADS), 0, s, dx, dy, dz, dt, di, (unsigned int)n, *filter,
                     counts);
  launch_filter_scan(counts, nb, h->compact.d_total(nb), s);
  hipLaunchKernelGGL(k_deskew_emit, dim3((unsigned)nb), dim3(DSK_THREADS), 0, s, dx, dy, dz, dt, di, (unsigned int)n, *filter, tab,
                     n_knots, counts, ox, oy, oz, di ? oi : nullptr, o_index, ucap);
  return compact_total(h, nb, cap, n_out);
}

// what every form checks before anything is written: the trajectory (into rows) and the sizes
int deskew_check(ndt_handle* h, size_t n, const double* knot_t, const double* knot_poses16, int n_knots, const double* ref16,
                 traj::KnotRow* rows) {
  if (n > (size_t)std::numeric_limits<int32_t>::max()) return fail(h, NDT_ERR_INVALID_ARG, "deskew: more than INT32_MAX points");
  const char* why = "";
  const int rc = traj::build_rows(knot_t, knot_poses16, n_knots, ref16, rows, &why);
  return rc ? fail(h, rc, why) : NDT_OK;
}

// a strided host cloud and its times -> the handle's device scratch [x | y | z | t | intensity] of n floats each, through
// the pinned staging (one transfer, enqueued on the engine's stream)
int deskew_upload(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, long intensity_offset_bytes, const float* t) {
  DeskewBufs& b = h->dsk;
  const bool has_i = intensity_offset_bytes >= 0;
  const size_t words = (has_i ? 5 : 4) * n;
  if (words > b.stage.cap) HIP_TRY(h, b.stage.ensure(5 * n + (5 * n) / 8 + 4096));
  HIP_TRY(h, b.in.ensure(5 * n));
  float* sx = b.stage.h, *sy = sx + n, *sz = sy + n, *st = sz + n, *si = st + n;
  gather_xyz(xyz, n, stride_bytes, sx, sy, sz);
  if (has_i) gather_column(xyz, n, stride_bytes, (size_t)intensity_offset_bytes, si);
  std::memcpy(st, t, n * sizeof(float));
  HIP_TRY(h, hipMemcpyAsync(b.in.p, b.stage.h, words * sizeof(float), hipMemcpyHostToDevice, h->stream));
  return NDT_OK;
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

int ndt_deskew_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, const float* d_intensity, const float* d_t,
                      size_t n, const double* knot_t, const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
                      const ndt_scan_filter* filter_or_null, float* ox, float* oy, float* oz, float* o_intensity,
                      int32_t* d_index_out, size_t cap, size_t* n_out) {
  if (!h || !n_out || ((!dx || !dy || !dz || !d_t) && n) || ((!ox || !oy || !oz) && cap && n)) return NDT_ERR_INVALID_ARG;
  traj::KnotRow rows[traj::MAX_KNOTS];
  int rc = deskew_check(h, n, knot_t, knot_poses16, n_knots, ref_pose16_or_null, rows);
  if (rc) return rc;
  if (o_intensity && !d_intensity) return fail(h, NDT_ERR_INVALID_ARG, "deskew: an intensity output without an intensity input");
  if (!filter_or_null && cap < n) {
    *n_out = n;
    return over_capacity(h, n);
  }
  {
    // compacting: the emit writes where other threads still read -- no output may overlap an input.  Aligned: a thread
    // reads element i of every input before it writes element i of every output, so an output may BE an input array
    // (same address), but must not overlap one in any other way.
    const size_t m = std::min(cap, n) * sizeof(float), nb = n * sizeof(float);
    const void* ins[5] = {dx, dy, dz, d_t, d_intensity};
    const void* outs[5] = {ox, oy, oz, o_intensity, d_index_out};
    for (const void* o : outs)
      for (const void* i : ins)
        if (ranges_overlap(o, m, i, nb) && (filter_or_null || o != i))
          return fail(h, NDT_ERR_INVALID_ARG, filter_or_null ? "deskew: a compacted output overlaps an input"
                                                             : "deskew: an output overlaps an input without being that array");
  }
  rc = bind_device(h);
  if (rc) return rc;
  return deskew_device(h, dx, dy, dz, d_intensity, d_t, n, rows, n_knots, filter_or_null, ox, oy, oz, o_intensity, d_index_out, cap,
                       n_out);
}

int ndt_deskew(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, long intensity_offset_bytes, const float* t,
               const double* knot_t, const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
               const ndt_scan_filter* filter_or_null, float* out, int32_t* index_out, size_t cap, size_t* n_out) {
  if (!h || !n_out || ((!xyz || !t) && n) || (!out && cap && n) || !layout_valid(stride_bytes, intensity_offset_bytes))
    return NDT_ERR_INVALID_ARG;
  traj::KnotRow rows[traj::MAX_KNOTS];
  int rc = deskew_check(h, n, knot_t, knot_poses16, n_knots, ref_pose16_or_null, rows);
  if (rc) return rc;
  if (!filter_or_null && cap < n) {
    *n_out = n;
    return over_capacity(h, n);
  }
  *n_out = 0;
  rc = bind_device(h);
  if (rc) return rc;
  if (n == 0) return NDT_OK;
  rc = deskew_upload(h, xyz, n, stride_bytes, intensity_offset_bytes, t);
  if (rc) return rc;
  DeskewBufs& b = h->dsk;
  const bool has_i = intensity_offset_bytes >= 0;
  HIP_TRY(h, b.out.ensure(4 * n));
  HIP_TRY(h, b.index.ensure(n));
  const float* in = b.in.p;
  float* o = b.out.p;
  rc = deskew_device(h, in, in + n, in + 2 * n, has_i ? in + 4 * n : nullptr, in + 3 * n, n, rows, n_knots, filter_or_null, o, o + n,
                     o + 2 * n, has_i ? o + 3 * n : nullptr, index_out ? b.index.p : nullptr, n, n_out);
  if (rc) return rc;
  // (the staging is free again: the upload out of it has been awaited)
  SideColumns side;
  side.d_i32 = b.index.p;
  side.i32_out = index_out;
  return download_strided(h, o, n, *n_out, cap, out, stride_bytes, intensity_offset_bytes, b.stage.h, side);
}

int ndt_keyframe_put_deskewed(ndt_handle* h, int64_t id, const float* xyz, size_t n, size_t stride_bytes,
                              long intensity_offset_bytes, const float* t, const double* knot_t, const double* knot_poses16,
                              int n_knots, const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null,
                              size_t* n_kept) {
  if (!h || ((!xyz || !t) && n) || !layout_valid(stride_bytes, intensity_offset_bytes)) return NDT_ERR_INVALID_ARG;
  traj::KnotRow rows[traj::MAX_KNOTS];
  int rc = deskew_check(h, n, knot_t, knot_poses16, n_knots, ref_pose16_or_null, rows);
  if (rc) return rc;
  rc = bind_device(h);
  if (rc) return rc;
  if (n) {
    rc = deskew_upload(h, xyz, n, stride_bytes, intensity_offset_bytes, t);
    if (rc) return rc;
  }
  // every argument error has been reported by now.  From here on only a HIP error (allocation, launch) can end the call
  // early, and it leaves keyframe `id` in the archive with no point (n = 0) -- never with the previous scan's count over
  // buffers that may have been re-allocated, never with a half-written scan that counts
  ndt_handle::Keyframe& kf = keyframe_claim(h, id, n);
  kf.n = 0;
  HIP_TRY(h, kf.x.ensure(n));
  HIP_TRY(h, kf.y.ensure(n));
  HIP_TRY(h, kf.z.ensure(n));
  const float* in = h->dsk.in.p;
  size_t m = 0;
  rc = deskew_device(h, in, in + n, in + 2 * n, intensity_offset_bytes >= 0 ? in + 4 * n : nullptr, in + 3 * n, n, rows, n_knots,
                     filter_or_null, kf.x.p, kf.y.p, kf.z.p, nullptr, nullptr, n, &m);
  if (rc) return rc;
  kf.n = m;
  if (n_kept) *n_kept = m;
  return NDT_OK;
}

}  // extern "C"
