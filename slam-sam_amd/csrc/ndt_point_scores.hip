// ndt_point_scores.hip -- per-point NDT scores and the score-based source filter (see ndt_engine.h).
//   ndt_score_points*        one launch of k_point_scores (ndt_derivs.hip) on the engine's stream; the kernel moves and
//                            classifies a point through ndt_neighbors_device.h, as the evaluation that scored it does
//   ndt_filter_source*       k_point_scores for the predicate values, then the stable compaction of
//                            ndt_compact_device.h in three small launches: k_filter_count, k_filter_scan, k_filter_emit.
// Integer counters only, no atomics: where a point lands depends on the points in front of it and on nothing else.
// Neither call touches the align state, the iteration history or the evaluation counters of the handle.
// This file also holds what every compaction of the engine shares beyond the device helpers: the one-block exclusive
// scan of the block counts (k_filter_scan, launch_filter_scan) and the host side (compact_scratch, compact_total).
#include "ndt_engine.h"
#include "ndt_compact_device.h"

namespace ndt {

namespace {

constexpr int FILT_THREADS = 256, FILT_WAVES = FILT_THREADS / 64;
constexpr int SCAN_THREADS = 1024, SCAN_WAVES = SCAN_THREADS / 64;

// the selection, exactly: v >= thr, or (keep_below) v < thr -- a point without a neighbour has v = 0
__device__ __forceinline__ bool filt_keep(double v, double thr, int keep_below) { return keep_below ? v < thr : v >= thr; }

__global__ void __launch_bounds__(FILT_THREADS) k_filter_count(const double* __restrict__ value, int n, double thr, int keep_below,
                                                              unsigned int* __restrict__ counts) {
  __shared__ unsigned int s_w[FILT_WAVES];
  const int i = (int)(blockIdx.x * FILT_THREADS + threadIdx.x);
  compact_ballot(i < n && filt_keep(value[i], thr, keep_below), s_w);
  __syncthreads();
  compact_block_count(s_w, counts);
}

// counts[0 .. nb) -> their exclusive prefix sums, in place; counts[nb] and *total receive the sum.  One block.
__global__ void __launch_bounds__(SCAN_THREADS) k_filter_scan(unsigned int* __restrict__ counts, int nb, unsigned int* __restrict__ total) {
  __shared__ unsigned int s_w[SCAN_WAVES];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  unsigned int carry = 0;   // block-uniform
  for (int base = 0; base < nb; base += SCAN_THREADS) {
    const int idx = base + (int)threadIdx.x;
    const unsigned int c = idx < nb ? counts[idx] : 0u;
    unsigned int incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned int v = __shfl_up(incl, off);
      if (lane >= off) incl += v;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    unsigned int wave_off = 0, chunk = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) {
      const unsigned int t = s_w[w];
      wave_off += w < wave ? t : 0u;
      chunk += t;
    }
    if (idx < nb) counts[idx] = carry + wave_off + incl - c;
    carry += chunk;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[nb] = carry;
    *total = carry;
  }
}

__global__ void __launch_bounds__(FILT_THREADS) k_filter_emit(const double* __restrict__ value, const float* __restrict__ sx,
                                                             const float* __restrict__ sy, const float* __restrict__ sz, int n,
                                                             double thr, int keep_below, const unsigned int* __restrict__ offsets,
                                                             float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz,
                                                             int* __restrict__ o_index, unsigned int cap) {
  __shared__ unsigned int s_w[FILT_WAVES];
  const int i = (int)(blockIdx.x * FILT_THREADS + threadIdx.x);
  const bool keep = i < n && filt_keep(value[i], thr, keep_below);
  const unsigned long long bal = compact_ballot(keep, s_w);
  __syncthreads();
  const unsigned int pos = compact_position(bal, s_w, offsets);
  if (keep && pos < cap) {   // (the output holds cap points: a selection beyond it is counted, not written)
    ox[pos] = sx[i];
    oy[pos] = sy[i];
    oz[pos] = sz[i];
    if (o_index) o_index[pos] = i;
  }
}

}  // namespace

void launch_filter_scan(unsigned int* d_counts, int nb, unsigned int* d_total, hipStream_t s) {
  hipLaunchKernelGGL(k_filter_scan, dim3(1), dim3(SCAN_THREADS), 0, s, d_counts, nb, d_total);
}

namespace engine {

int compact_scratch(ndt_handle* h, int nb) {
  HIP_TRY(h, h->compact.counts.ensure((size_t)nb + 2));
  HIP_TRY(h, h->compact.total_h.ensure(4));
  return NDT_OK;
}

int compact_total(ndt_handle* h, int nb, size_t cap, size_t* n_out) {
  CompactBufs& c = h->compact;
  HIP_TRY(h, hipGetLastError());   // (of the three launches)
  HIP_TRY(h, hipMemcpyAsync(c.total_h.h, c.d_total(nb), sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  *n_out = (size_t)c.total_h.h[0];
  return *n_out > cap ? over_capacity(h, *n_out) : NDT_OK;
}

namespace {

// as ndt_score_transform: a pending deferred build is settled, then target and source are asked for
int points_ready(ndt_handle* h) {
  int rc = bind_device(h);
  if (rc) return rc;
  return ready_for_eval(h);
}

// k_point_scores at T into device arrays (each may be null); enqueued on the engine's stream, not awaited
int enqueue_point_scores(ndt_handle* h, const float T[16], double* d_score, double* d_best, int32_t* d_npairs, int64_t* d_cell) {
  if (h->n_src == 0 || (!d_score && !d_best && !d_npairs && !d_cell)) return NDT_OK;
  if (h->n_src > (size_t)std::numeric_limits<int>::max() - FILT_THREADS) return fail(h, NDT_ERR_INVALID_ARG, "source too large");
  EvalConsts ec = make_eval_consts(h, false);
  ec.score_only = 1;
  const VoxelRecord* records = nullptr;
  int rc = records_for_eval(h, &ec, &records);
  if (rc) return rc;
  PoseConsts pc{};   // (R|t only: a score needs no angle tables)
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pc.R[3 * i + j] = T[4 * j + i];
    pc.t[i] = T[12 + i];
  }
  static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "output types");
  // the source as handed over (vx / vy / vz), never the block-sorted copy: outputs line up with the caller's cloud
  launch_point_scores(h->vx, h->vy, h->vz, h->n_src, h->geom, h->cell2leaf.p, records, pc, ec, d_score, d_best, d_npairs,
                      reinterpret_cast<long long*>(d_cell), h->stream);
  HIP_TRY(h, hipGetLastError());
  return NDT_OK;
}

int filter_device(ndt_handle* h, const float T[16], double min_score, int keep_below, float* ox, float* oy, float* oz,
                  int32_t* d_index, size_t cap, size_t* n_out) {
  const size_t n = h->n_src;
  if (n == 0) return NDT_OK;   // (an empty shard of a sharded source)
  const int nb = (int)((n + FILT_THREADS - 1) / FILT_THREADS), below = keep_below ? 1 : 0;
  HIP_TRY(h, h->ps.best.ensure(n));
  int rc = compact_scratch(h, nb);
  if (rc) return rc;
  rc = enqueue_point_scores(h, T, nullptr, h->ps.best.p, nullptr, nullptr);
  if (rc) return rc;
  hipStream_t s = h->stream;
  const double* value = h->ps.best.p;
  unsigned int* counts = h->compact.counts.p;
  const unsigned int ucap = (unsigned int)std::min<size_t>(cap, n);
  hipLaunchKernelGGL(k_filter_count, dim3((unsigned)nb), dim3(FILT_THREADS), 0, s, value, (int)n, min_score, below, counts);
  launch_filter_scan(counts, nb, h->compact.d_total(nb), s);
  hipLaunchKernelGGL(k_filter_emit, dim3((unsigned)nb), dim3(FILT_THREADS), 0, s, value, h->vx, h->vy, h->vz, (int)n, min_score,
                     below, counts, ox, oy, oz, d_index, ucap);
  return compact_total(h, nb, cap, n_out);
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

int64_t ndt_source_size(const ndt_handle* h) { return h ? (int64_t)h->n_src : NDT_ERR_INVALID_ARG; }

int ndt_score_points_device(ndt_handle* h, const float T[16], double* d_score, double* d_nearest_voxel_score,
                            int32_t* d_n_neighbors, int64_t* d_best_voxel, size_t cap) {
  if (!h || !T) return NDT_ERR_INVALID_ARG;
  int rc = points_ready(h);
  if (rc) return rc;
  if ((d_score || d_nearest_voxel_score || d_n_neighbors || d_best_voxel) && cap < h->n_src)
    return fail(h, NDT_ERR_INVALID_ARG, "score points: an output holds fewer than n_source");
  rc = enqueue_point_scores(h, T, d_score, d_nearest_voxel_score, d_n_neighbors, d_best_voxel);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NDT_OK;
}

int ndt_score_points(ndt_handle* h, const float T[16], double* score, double* nearest_voxel_score, int32_t* n_neighbors,
                     int64_t* best_voxel, size_t cap) {
  if (!h || !T) return NDT_ERR_INVALID_ARG;
  int rc = points_ready(h);
  if (rc) return rc;
  const size_t n = h->n_src;
  if ((score || nearest_voxel_score || n_neighbors || best_voxel) && cap < n)
    return fail(h, NDT_ERR_INVALID_ARG, "score points: an output holds fewer than n_source");
  if (n == 0) return NDT_OK;
  PointScoreBufs& ps = h->ps;
  if (score) HIP_TRY(h, ps.score.ensure(n));
  if (nearest_voxel_score) HIP_TRY(h, ps.best.ensure(n));
  if (n_neighbors) HIP_TRY(h, ps.npairs.ensure(n));
  if (best_voxel) HIP_TRY(h, ps.cell.ensure(n));
  rc = enqueue_point_scores(h, T, score ? ps.score.p : nullptr, nearest_voxel_score ? ps.best.p : nullptr,
                            n_neighbors ? ps.npairs.p : nullptr, best_voxel ? reinterpret_cast<int64_t*>(ps.cell.p) : nullptr);
  if (rc) return rc;
  hipStream_t s = h->stream;
  if (score) HIP_TRY(h, hipMemcpyAsync(score, ps.score.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (nearest_voxel_score) HIP_TRY(h, hipMemcpyAsync(nearest_voxel_score, ps.best.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (n_neighbors) HIP_TRY(h, hipMemcpyAsync(n_neighbors, ps.npairs.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (best_voxel) HIP_TRY(h, hipMemcpyAsync(best_voxel, ps.cell.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return NDT_OK;
}

int ndt_filter_source_device(ndt_handle* h, const float T[16], double min_score, int keep_below, float* ox, float* oy, float* oz,
                             int32_t* d_index_out, size_t cap, size_t* n_out) {
  if (!h || !T || !n_out || ((!ox || !oy || !oz) && cap) || std::isnan(min_score)) return NDT_ERR_INVALID_ARG;
  *n_out = 0;
  int rc = points_ready(h);
  if (rc) return rc;
  return filter_device(h, T, min_score, keep_below, ox, oy, oz, d_index_out, cap, n_out);
}

int ndt_filter_source(ndt_handle* h, const float T[16], double min_score, int keep_below, float* out_xyz, int32_t* index_out,
                      size_t cap_points, size_t* n_out) {
  if (!h || !T || !n_out || (!out_xyz && cap_points) || std::isnan(min_score)) return NDT_ERR_INVALID_ARG;
  *n_out = 0;
  int rc = points_ready(h);
  if (rc) return rc;
  const size_t n = h->n_src;
  if (n == 0) return NDT_OK;
  PointScoreBufs& ps = h->ps;
  HIP_TRY(h, ps.out.ensure(3 * n));
  HIP_TRY(h, ps.index.ensure(n));
  rc = filter_device(h, T, min_score, keep_below, ps.out.p, ps.out.p + n, ps.out.p + 2 * n, ps.index.p, n, n_out);
  if (rc) return rc;
  // (a tight cloud is a stride of 12 bytes without intensity)
  SideColumns side;
  side.d_i32 = ps.index.p;
  side.i32_out = index_out;
  return download_strided(h, ps.out.p, n, *n_out, cap_points, out_xyz, 3 * sizeof(float), -1, nullptr, side);
}

}  // extern "C"
