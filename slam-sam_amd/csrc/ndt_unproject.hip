// ndt_unproject.hip -- a lidar range image to points through the scan model's tables, with the range gate, the
// acquisition filter and the deskew in the same pass (include/ndt_hip.h has the contract, DESIGN 7h the figures).
//   organised  (no filter)  ONE launch of k_unproject_aligned: out[i] = pixel i, an invalid pixel -> NaN
//   compacting (filter)     the stable compaction of ndt_compact_device.h in three launches: k_unproject_count
//                           (valid && kept), the one-block scan (launch_filter_scan), k_unproject_emit (the moved point
//                           behind its offset)
// One thread per pixel, pixel i = col * n_rows + row: the u32 range, the u8 reflectivity and the three direction tables
// are read at i by consecutive lanes (coalesced; a wave's 64 reflectivity bytes are one 64-byte line).  A block's 256
// pixels lie in at most 256 columns: the block reads the time and the three offsets of each of ITS columns once into LDS
// (coalesced as well), and a pixel takes them from there.  The knot table sits in LDS as in ndt_deskew.hip; the
// predicate and the motion ARE that file's (ndt_deskew_device.h).  Integer offsets only, no atomics.  Everything on the
// engine's stream; the target, the source, the align state, the history and the counters of the handle are not touched.
#include "ndt_engine.h"
#include "ndt_compact_device.h"
#include "ndt_deskew_device.h"
#include "ndt_trajectory.h"

namespace ndt {

namespace {

// what every kernel takes: the range image, the model's tables and the gate
struct UnpArgs {
  const uint32_t* range;
  const uint8_t* refl;    // nullable
  const float* col_t;
  const float *x1, *y1, *z1, *x2, *y2, *z2;
  unsigned int n_rows, n;             // n = n_cols * n_rows pixels
  unsigned int row_step;              // <= 1: every row
  int use_range;
  float range_min, range_max;
};

// a block's columns: time and offsets of column c0 + k
struct UnpCols {
  float t[DSK_THREADS], x[DSK_THREADS], y[DSK_THREADS], z[DSK_THREADS];
};

// loads the columns of the block's pixels; the caller's next barrier publishes them.  Returns the first column.
__device__ __forceinline__ unsigned int unp_load_cols(const UnpArgs& a, UnpCols& s) {
  const unsigned int first = blockIdx.x * DSK_THREADS, last = min(first + DSK_THREADS - 1u, a.n - 1u);
  const unsigned int c0 = first / a.n_rows, c1 = last / a.n_rows;   // (first < n: the grid has ceil(n / 256) blocks)
  const unsigned int c = c0 + threadIdx.x;
  if (c <= c1) {
    s.t[threadIdx.x] = a.col_t[c];
    s.x[threadIdx.x] = a.x2[c];
    s.y[threadIdx.x] = a.y2[c];
    s.z[threadIdx.x] = a.z2[c];
  }
  return c0;
}

// pixel i < n: its raw point (NaN where it is not valid), time and intensity; returns `valid` of the header
__device__ __forceinline__ bool unp_pixel(const UnpArgs& a, const UnpCols& s, unsigned int c0, unsigned int i, float* x, float* y,
                                          float* z, float* t, float* inten) {
  const unsigned int col = i / a.n_rows, row = i - col * a.n_rows, k = col - c0;
  const uint32_t r = a.range[i];
  *t = s.t[k];
  *inten = a.refl ? (float)a.refl[i] : 0.0f;
  const float range_m = (float)r * 0.001f;
  const bool valid = r != 0u && isfinite(*t) && (a.row_step <= 1u || row % a.row_step == 0u) &&
                     (!a.use_range || (a.range_min <= range_m && range_m <= a.range_max));
  if (valid) {
    *x = __fmaf_rn(range_m, a.x1[i], s.x[k]);
    *y = __fmaf_rn(range_m, a.y1[i], s.y[k]);
    *z = __fmaf_rn(range_m, a.z1[i], s.z[k]);
  } else {
    *x = *y = *z = __builtin_nanf("");
  }
  return valid;
}

// the deskew's predicate on the raw point, its intensity array being this pixel's (float)reflectivity -- or none (two
// calls: the address of a local chosen at run time would put it into scratch)
__device__ __forceinline__ bool unp_keep(const UnpArgs& a, const ndt_scan_filter& f, float x, float y, float z, float t, float inten) {
  return a.refl ? dsk_keep(f, x, y, z, t, &inten, 0) : dsk_keep(f, x, y, z, t, nullptr, 0);
}

__global__ void __launch_bounds__(DSK_THREADS) k_unproject_aligned(UnpArgs a, const double* __restrict__ table, int n_knots,
                                                                  float* __restrict__ ox, float* __restrict__ oy,
                                                                  float* __restrict__ oz, float* __restrict__ oi,
                                                                  float* __restrict__ ot, int* __restrict__ o_index) {
  __shared__ double s_tab[traj::MAX_KNOTS * traj::ROW_WORDS];
  __shared__ UnpCols s_cols;
  const unsigned int c0 = unp_load_cols(a, s_cols);
  dsk_load_table(table, n_knots, s_tab);   // (its barrier also publishes s_cols)
  const unsigned int i = blockIdx.x * DSK_THREADS + threadIdx.x;
  if (i >= a.n) return;
  float x, y, z, t, inten;
  unp_pixel(a, s_cols, c0, i, &x, &y, &z, &t, &inten);
  if (n_knots > 0) {   // as k_deskew_aligned treats the raw point: moved where it is finite, NaN where it is not
    if (isfinite(x) && isfinite(y) && isfinite(z) && isfinite(t)) {
      dsk_move(reinterpret_cast<const traj::KnotRow*>(s_tab), n_knots, x, y, z, t, &x, &y, &z);
    } else {
      x = y = z = __builtin_nanf("");
    }
  }
  ox[i] = x;
  oy[i] = y;
  oz[i] = z;
  if (oi) oi[i] = inten;
  if (ot) ot[i] = t;
  if (o_index) o_index[i] = (int)i;
}

__global__ void __launch_bounds__(DSK_THREADS) k_unproject_count(UnpArgs a, ndt_scan_filter f, unsigned int* __restrict__ counts) {
  __shared__ UnpCols s_cols;
  __shared__ unsigned int s_w[DSK_WAVES];
  const unsigned int c0 = unp_load_cols(a, s_cols);
  __syncthreads();
  const unsigned int i = blockIdx.x * DSK_THREADS + threadIdx.x;
  bool keep = false;
  if (i < a.n) {
    float x, y, z, t, inten;
    keep = unp_pixel(a, s_cols, c0, i, &x, &y, &z, &t, &inten) && unp_keep(a, f, x, y, z, t, inten);
  }
  compact_ballot(keep, s_w);
  __syncthreads();
  compact_block_count(s_w, counts);
}

__global__ void __launch_bounds__(DSK_THREADS) k_unproject_emit(UnpArgs a, ndt_scan_filter f, const double* __restrict__ table,
                                                               int n_knots, const unsigned int* __restrict__ offsets,
                                                               float* __restrict__ ox, float* __restrict__ oy,
                                                               float* __restrict__ oz, float* __restrict__ oi,
                                                               float* __restrict__ ot, int* __restrict__ o_index,
                                                               unsigned int cap) {
  __shared__ double s_tab[traj::MAX_KNOTS * traj::ROW_WORDS];
  __shared__ UnpCols s_cols;
  __shared__ unsigned int s_w[DSK_WAVES];
  const unsigned int c0 = unp_load_cols(a, s_cols);
  dsk_load_table(table, n_knots, s_tab);   // (its barrier also publishes s_cols)
  const unsigned int i = blockIdx.x * DSK_THREADS + threadIdx.x;
  float x = 0.0f, y = 0.0f, z = 0.0f, t = 0.0f, inten = 0.0f;
  bool keep = false;
  if (i < a.n) keep = unp_pixel(a, s_cols, c0, i, &x, &y, &z, &t, &inten) && unp_keep(a, f, x, y, z, t, inten);
  const unsigned long long bal = compact_ballot(keep, s_w);
  __syncthreads();
  const unsigned int pos = compact_position(bal, s_w, offsets);
  if (keep && pos < cap) {   // (the output holds cap points: a selection beyond it is counted, not written)
    if (n_knots > 0) dsk_move(reinterpret_cast<const traj::KnotRow*>(s_tab), n_knots, x, y, z, t, &x, &y, &z);
    ox[pos] = x;
    oy[pos] = y;
    oz[pos] = z;
    if (oi) oi[pos] = inten;
    if (ot) ot[pos] = t;
    if (o_index) o_index[pos] = (int)i;
  }
}

}  // namespace

namespace engine {
namespace {

size_t unp_pixels(const ndt_handle* h) { return (size_t)h->scan.n_cols * (size_t)h->scan.n_rows; }

}  // namespace

// The trajectory's table to the device (knots_upload), then the launches; awaited.  Every pointer but `rows` is device
// memory.  Arguments have been checked.
int unproject_device(ndt_handle* h, const uint32_t* d_range, const uint8_t* d_refl, const float* d_col_t, const ndt_range_gate* gate,
                     const traj::KnotRow* rows, int n_knots, const ndt_scan_filter* filter, float* ox, float* oy, float* oz, float* oi,
                     float* ot, int32_t* o_index, size_t cap, size_t* n_out) {
  *n_out = 0;
  ScanModelBufs& b = h->scan;
  hipStream_t s = h->stream;
  const size_t n = unp_pixels(h);
  int rc = knots_upload(h, rows, n_knots);
  if (rc) return rc;
  const double* tab = h->knots.tab.p;
  UnpArgs a;
  a.range = d_range; a.refl = d_refl; a.col_t = d_col_t;
  a.x1 = b.dir.p; a.y1 = b.dir.p + n; a.z1 = b.dir.p + 2 * n;
  a.x2 = b.off.p; a.y2 = b.off.p + b.n_cols; a.z2 = b.off.p + 2 * (size_t)b.n_cols;
  a.n_rows = (unsigned int)b.n_rows; a.n = (unsigned int)n;
  a.row_step = gate ? (unsigned int)gate->row_step : 0u;
  a.use_range = gate ? gate->use_range : 0;
  a.range_min = gate ? gate->range_min : 0.0f;
  a.range_max = gate ? gate->range_max : 0.0f;
  const int nb = (int)((n + DSK_THREADS - 1) / DSK_THREADS);
  static_assert(sizeof(int) == sizeof(int32_t), "index type");
  if (!filter) {
    hipLaunchKernelGGL(k_unproject_aligned, dim3((unsigned)nb), dim3(DSK_THREADS), 0, s, a, tab, n_knots, ox, oy, oz, oi, ot,
                       o_index);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));
    *n_out = n;
    return NDT_OK;
  }
  rc = compact_scratch(h, nb);
  if (rc) return rc;
  unsigned int* counts = h->compact.counts.p;
  const unsigned int ucap = (unsigned int)std::min<size_t>(cap, n);
  hipLaunchKernelGGL(k_unproject_count, dim3((unsigned)nb), dim3(DSK_THREADS), 0, s, a, *filter, counts);
  launch_filter_scan(counts, nb, h->compact.d_total(nb), s);
  hipLaunchKernelGGL(k_unproject_emit, dim3((unsigned)nb), dim3(DSK_THREADS), 0, s, a, *filter, tab, n_knots, counts, ox, oy, oz, oi,
                     ot, o_index, ucap);
  return compact_total(h, nb, cap, n_out);
}

// what every form checks before anything is written: the model, the gate and the trajectory (into rows; n_knots = 0
// with no trajectory pointer: no motion, rows stays unused)
int unproject_check(ndt_handle* h, const ndt_range_gate* gate, const double* knot_t, const double* knot_poses16, int n_knots,
                    const double* ref16, traj::KnotRow* rows) {
  if (h->scan.n_cols == 0) return fail(h, NDT_ERR_INVALID_ARG, "unproject: no scan model set (ndt_scan_model_set)");
  if (gate) {
    if (gate->row_step < 0) return fail(h, NDT_ERR_INVALID_ARG, "unproject: row_step is negative");
    if (gate->use_range && !(gate->range_min <= gate->range_max))
      return fail(h, NDT_ERR_INVALID_ARG, "unproject: range gate with range_min > range_max");
  }
  if (n_knots == 0 && !knot_t && !knot_poses16 && !ref16) return NDT_OK;   // no motion
  const char* why = "";
  const int rc = traj::build_rows(knot_t, knot_poses16, n_knots, ref16, rows, &why);
  return rc ? fail(h, rc, why) : NDT_OK;
}

namespace {

size_t unp_stage_words(size_t n, size_t n_cols) { return n + n_cols + (n + 3) / 4; }

// a host range image -> the handle's device scratch [range_mm | col_t | reflectivity] through the pinned staging: ONE
// transfer, enqueued on the engine's stream
int unproject_upload(ndt_handle* h, const uint32_t* range_mm, const uint8_t* reflectivity, const float* col_t) {
  ScanModelBufs& b = h->scan;
  const size_t n = unp_pixels(h), nc = (size_t)b.n_cols;
  const size_t words = reflectivity ? unp_stage_words(n, nc) : n + nc;
  // (the staging also carries the result down: 5 floats per point)
  HIP_TRY(h, b.stage.ensure(5 * n + 64));
  HIP_TRY(h, b.in.ensure(unp_stage_words(n, nc)));
  std::memcpy(b.stage.h, range_mm, n * sizeof(uint32_t));
  std::memcpy(b.stage.h + n, col_t, nc * sizeof(float));
  if (reflectivity) std::memcpy(b.stage.h + n + nc, reflectivity, n);
  HIP_TRY(h, hipMemcpyAsync(b.in.p, b.stage.h, words * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  return NDT_OK;
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

int ndt_scan_model_set(ndt_handle* h, int n_cols, int n_rows, const float* x1, const float* y1, const float* z1, const float* x2,
                       const float* y2, const float* z2) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (!x1 || !y1 || !z1 || !x2 || !y2 || !z2) return fail(h, NDT_ERR_INVALID_ARG, "scan model: a table pointer is NULL");
  if (n_cols < 1 || n_rows < 1 || (int64_t)n_cols * n_rows > (int64_t)std::numeric_limits<int32_t>::max())
    return fail(h, NDT_ERR_INVALID_ARG, "scan model: n_cols and n_rows must be at least 1 and n_cols * n_rows at most INT32_MAX");
  int rc = bind_device(h);
  if (rc) return rc;
  ScanModelBufs& b = h->scan;
  const size_t n = (size_t)n_cols * (size_t)n_rows, nc = (size_t)n_cols;
  b.n_cols = b.n_rows = 0;   // (a HIP error below leaves no model rather than half of one)
  h->pkt.drop();             // the packet format is the model's shape: gone with it, and any frame in progress
  HIP_TRY(h, b.dir.ensure(3 * n));
  HIP_TRY(h, b.off.ensure(3 * nc));
  const float* dir[3] = {x1, y1, z1};
  const float* off[3] = {x2, y2, z2};
  for (int a = 0; a < 3; ++a) {
    HIP_TRY(h, hipMemcpyAsync(b.dir.p + (size_t)a * n, dir[a], n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(b.off.p + (size_t)a * nc, off[a], nc * sizeof(float), hipMemcpyHostToDevice, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  b.n_cols = n_cols;
  b.n_rows = n_rows;
  return NDT_OK;
}

int ndt_scan_model_clear(ndt_handle* h) {
  if (!h) return NDT_ERR_INVALID_ARG;
  h->scan.n_cols = h->scan.n_rows = 0;   // (the buffers stay for the next model)
  h->pkt.drop();
  return NDT_OK;
}

int ndt_scan_model_get_info(const ndt_handle* h, int* n_cols, int* n_rows) {
  if (!h || !n_cols || !n_rows) return NDT_ERR_INVALID_ARG;
  *n_cols = h->scan.n_cols;
  *n_rows = h->scan.n_rows;
  return NDT_OK;
}

int ndt_unproject_device(ndt_handle* h, const uint32_t* d_range_mm, const uint8_t* d_reflectivity, const float* d_col_t,
                         const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16, int n_knots,
                         const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* ox, float* oy, float* oz,
                         float* o_intensity, float* o_t, int32_t* d_index_out, size_t cap, size_t* n_out) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (!n_out) return fail(h, NDT_ERR_INVALID_ARG, "unproject: n_out is NULL");
  traj::KnotRow rows[traj::MAX_KNOTS];
  int rc = unproject_check(h, gate_or_null, knot_t, knot_poses16, n_knots, ref_pose16_or_null, rows);
  if (rc) return rc;
  if (!d_range_mm || !d_col_t) return fail(h, NDT_ERR_INVALID_ARG, "unproject: the range image or the column times are NULL");
  if ((!ox || !oy || !oz) && cap) return fail(h, NDT_ERR_INVALID_ARG, "unproject: an output coordinate array is NULL");
  if (o_intensity && !d_reflectivity) return fail(h, NDT_ERR_INVALID_ARG, "unproject: an intensity output without a reflectivity input");
  const size_t n = unp_pixels(h);
  if (!filter_or_null && cap < n) {
    *n_out = n;
    return over_capacity(h, n);
  }
  {
    // inputs and outputs differ in type and layout: no output may overlap an input in either form
    const size_t m = std::min(cap, n) * sizeof(float);
    const void* ins[3] = {d_range_mm, d_reflectivity, d_col_t};
    const size_t in_bytes[3] = {n * sizeof(uint32_t), n, (size_t)h->scan.n_cols * sizeof(float)};
    const void* outs[6] = {ox, oy, oz, o_intensity, o_t, d_index_out};
    for (const void* o : outs)
      for (int i = 0; i < 3; ++i)
        if (ranges_overlap(o, m, ins[i], in_bytes[i])) return fail(h, NDT_ERR_INVALID_ARG, "unproject: an output overlaps an input");
    // ... and the kernels take the outputs as distinct arrays (__restrict__)
    for (int a = 0; a < 6; ++a)
      for (int b = a + 1; b < 6; ++b)
        if (ranges_overlap(outs[a], m, outs[b], m)) return fail(h, NDT_ERR_INVALID_ARG, "unproject: two outputs overlap");
  }
  rc = bind_device(h);
  if (rc) return rc;
  return unproject_device(h, d_range_mm, d_reflectivity, d_col_t, gate_or_null, rows, n_knots, filter_or_null, ox, oy, oz, o_intensity,
                          o_t, d_index_out, cap, n_out);
}

int ndt_unproject(ndt_handle* h, const uint32_t* range_mm, const uint8_t* reflectivity, const float* col_t,
                  const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16, int n_knots,
                  const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* out, size_t stride_bytes,
                  long intensity_offset_bytes, float* t_out, int32_t* index_out, size_t cap, size_t* n_out) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (!n_out) return fail(h, NDT_ERR_INVALID_ARG, "unproject: n_out is NULL");
  traj::KnotRow rows[traj::MAX_KNOTS];
  int rc = unproject_check(h, gate_or_null, knot_t, knot_poses16, n_knots, ref_pose16_or_null, rows);
  if (rc) return rc;
  if (!range_mm || !col_t) return fail(h, NDT_ERR_INVALID_ARG, "unproject: the range image or the column times are NULL");
  if (!out && cap) return fail(h, NDT_ERR_INVALID_ARG, "unproject: the output cloud is NULL");
  if (!layout_valid(stride_bytes, intensity_offset_bytes)) return fail(h, NDT_ERR_INVALID_ARG, "unproject: invalid output layout");
  const bool has_i = intensity_offset_bytes >= 0;
  if (has_i && !reflectivity) return fail(h, NDT_ERR_INVALID_ARG, "unproject: an intensity output without a reflectivity input");
  const size_t n = unp_pixels(h), nc = (size_t)h->scan.n_cols;
  if (!filter_or_null && cap < n) {
    *n_out = n;
    return over_capacity(h, n);
  }
  *n_out = 0;
  rc = bind_device(h);
  if (rc) return rc;
  rc = unproject_upload(h, range_mm, reflectivity, col_t);
  if (rc) return rc;
  ScanModelBufs& b = h->scan;
  HIP_TRY(h, b.out.ensure(5 * n));
  HIP_TRY(h, b.index.ensure(n));
  float* o = b.out.p;
  rc = unproject_device(h, b.in.p, reflectivity ? reinterpret_cast<const uint8_t*>(b.in.p + n + nc) : nullptr,
                        reinterpret_cast<const float*>(b.in.p + n), gate_or_null, rows, n_knots, filter_or_null, o, o + n, o + 2 * n,
                        has_i ? o + 3 * n : nullptr, t_out ? o + 4 * n : nullptr, index_out ? b.index.p : nullptr, n, n_out);
  if (rc) return rc;
  // (the staging is free again: the upload out of it has been awaited)
  SideColumns side;
  side.d_f32 = o + 4 * n;
  side.f32_out = t_out;
  side.d_i32 = b.index.p;
  side.i32_out = index_out;
  return download_strided(h, o, n, *n_out, cap, out, stride_bytes, intensity_offset_bytes, reinterpret_cast<float*>(b.stage.h), side);
}

int ndt_keyframe_put_from_ranges(ndt_handle* h, int64_t id, const uint32_t* range_mm, const uint8_t* reflectivity, const float* col_t,
                                 const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16, int n_knots,
                                 const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, size_t* n_kept) {
  if (!h) return NDT_ERR_INVALID_ARG;
  traj::KnotRow rows[traj::MAX_KNOTS];
  int rc = unproject_check(h, gate_or_null, knot_t, knot_poses16, n_knots, ref_pose16_or_null, rows);
  if (rc) return rc;
  if (!range_mm || !col_t) return fail(h, NDT_ERR_INVALID_ARG, "unproject: the range image or the column times are NULL");
  rc = bind_device(h);
  if (rc) return rc;
  rc = unproject_upload(h, range_mm, reflectivity, col_t);
  if (rc) return rc;
  const ndt_scan_filter keep_valid{};   // an archive holds no NaN points: no filter = the zeroed one
  const size_t n = unp_pixels(h), nc = (size_t)h->scan.n_cols;
  // every argument error has been reported by now.  From here on only a HIP error (allocation, launch) can end the call
  // early, and it leaves keyframe `id` in the archive with no point (n = 0), as ndt_keyframe_put_deskewed does
  ndt_handle::Keyframe& kf = keyframe_claim(h, id, n);
  kf.n = 0;
  HIP_TRY(h, kf.x.ensure(n));
  HIP_TRY(h, kf.y.ensure(n));
  HIP_TRY(h, kf.z.ensure(n));
  const uint32_t* in = h->scan.in.p;
  size_t m = 0;
  rc = unproject_device(h, in, reflectivity ? reinterpret_cast<const uint8_t*>(in + n + nc) : nullptr,
                        reinterpret_cast<const float*>(in + n), gate_or_null, rows, n_knots, filter_or_null ? filter_or_null : &keep_valid,
                        kf.x.p, kf.y.p, kf.z.p, nullptr, nullptr, nullptr, n, &m);
  if (rc) return rc;
  kf.n = m;
  if (n_kept) *n_kept = m;
  return NDT_OK;
}

}  // extern "C"
