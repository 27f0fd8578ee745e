// ndt_point_scores.hip -- per-point NDT scores and the score-based source filter (see ndt_engine.h).
//   ndt_score_points*        one launch of k_point_scores (ndt_derivs.hip) on the engine's stream
//   ndt_filter_source*       k_point_scores for the predicate values, then a stable compaction in three small launches:
//                            per-block counts (wave ballots + popcounts), an exclusive scan of the counts by ONE block,
//                            and the emit (the ballots again, a per-block exclusive scan of the wave counts in LDS).
// Integer counters only, no atomics: where a point lands depends on the points in front of it and on nothing else.
// Neither call touches the align state, the iteration history or the evaluation counters of the handle.
#include "ndt_engine.h"

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
  const bool keep = i < n && filt_keep(value[i], thr, keep_below);
  const unsigned long long bal = __ballot(keep);
  if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = (unsigned int)__popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int c = 0;
#pragma unroll
    for (int w = 0; w < FILT_WAVES; ++w) c += s_w[w];
    counts[blockIdx.x] = c;
  }
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
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const bool keep = i < n && filt_keep(value[i], thr, keep_below);
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) s_w[wave] = (unsigned int)__popcll(bal);
  __syncthreads();
  unsigned int wave_off = 0;
#pragma unroll
  for (int w = 0; w < FILT_WAVES; ++w) wave_off += w < wave ? s_w[w] : 0u;
  const unsigned int rank = (unsigned int)__popcll(bal & ((1ull << lane) - 1ull));
  const unsigned int pos = offsets[blockIdx.x] + wave_off + rank;
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

int filter_blocks(size_t n) { return (int)((n + FILT_THREADS - 1) / FILT_THREADS); }

void launch_filter_compact(const double* d_value, const float* sx, const float* sy, const float* sz, size_t n, double thr,
                           int keep_below, unsigned int* d_block_counts, unsigned int* d_total, float* ox, float* oy, float* oz,
                           int* o_index, size_t cap, hipStream_t s) {
  if (n == 0) return;
  const int nb = filter_blocks(n);
  const unsigned int ucap = (unsigned int)std::min<size_t>(cap, n);
  hipLaunchKernelGGL(k_filter_count, dim3((unsigned)nb), dim3(FILT_THREADS), 0, s, d_value, (int)n, thr, keep_below, d_block_counts);
  launch_filter_scan(d_block_counts, nb, d_total, s);
  hipLaunchKernelGGL(k_filter_emit, dim3((unsigned)nb), dim3(FILT_THREADS), 0, s, d_value, sx, sy, sz, (int)n, thr, keep_below,
                     d_block_counts, ox, oy, oz, o_index, ucap);
}

namespace engine {
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
  PointScoreBufs& ps = h->ps;
  HIP_TRY(h, ps.best.ensure(n));
  HIP_TRY(h, ps.counts.ensure((size_t)filter_blocks(n) + 2));
  int rc = enqueue_point_scores(h, T, nullptr, ps.best.p, nullptr, nullptr);
  if (rc) return rc;
  unsigned int* d_total = ps.counts.p + filter_blocks(n) + 1;
  launch_filter_compact(ps.best.p, h->vx, h->vy, h->vz, n, min_score, keep_below ? 1 : 0, ps.counts.p, d_total, ox, oy, oz,
                        d_index, cap, h->stream);
  HIP_TRY(h, hipGetLastError());
  unsigned int total = 0;
  HIP_TRY(h, hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  *n_out = (size_t)total;
  if (*n_out > cap) return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(*n_out) + " points selected");
  return NDT_OK;
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
  const size_t m = *n_out;
  if (m > cap_points) return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(m) + " points selected");
  if (m == 0) return NDT_OK;
  std::vector<float> back(3 * m);
  for (int a = 0; a < 3; ++a)
    HIP_TRY(h, hipMemcpyAsync(back.data() + (size_t)a * m, ps.out.p + (size_t)a * n, m * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (index_out) HIP_TRY(h, hipMemcpyAsync(index_out, ps.index.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < m; ++i) {
    out_xyz[3 * i + 0] = back[i];
    out_xyz[3 * i + 1] = back[m + i];
    out_xyz[3 * i + 2] = back[2 * m + i];
  }
  return NDT_OK;
}

}  // extern "C"
