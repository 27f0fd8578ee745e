// ndt_d2d.hip -- distribution-to-distribution NDT (Stoyanov et al. 2012): a submap's voxels registered to the target's
// (see ndt_engine.h; the rule is stated in include/ndt_hip.h).
//   ndt_set_source_distributions*   the records of ndt_map_export_state* are kept; k_d2d_finalize puts each through the
//                                   target build's own finalize_leaf (ndt_leaf_device.h) and counts what it accepts per
//                                   block, k_filter_scan turns the counts into offsets, k_d2d_emit writes the accepted
//                                   Gaussians {mean 3, cov 6} in input order (ndt_compact_device.h)
//   ndt_eval_derivatives_d2d        k_d2d_gather_target once per published target (mean 3 + cov 6 per leaf slot, from
//                                   `stats`), then per pose one launch of k_d2d_eval<HESSIAN> -- one source Gaussian per
//                                   lane -- and one launch of the fixed-order sum over all poses
//   ndt_align_d2d                   newton_align over that evaluation
// A moved mean's neighbours are found by ndt_neighbors_device.h, as every evaluator's.  Sums: lane -> wave -> block -> one
// row per block (eval_block_row, ndt_evalrows_device.h) -> k_eval_rows_sum in fixed order; the host side around the
// launches (lane_eval_rows, finish_words, lane_align) is ndt_eval_rows.hip's, shared with the continuous-time evaluation.
// The point source, the align state and the iteration history of the handle are not touched.
#include "ndt_engine.h"
#include "ndt_compact_device.h"
#include "ndt_d2d_device.h"
#include "ndt_evalrows_device.h"
#include "ndt_leaf_device.h"
#include "ndt_neighbors_device.h"

namespace ndt {

namespace {

constexpr int D2D_THREADS = 256, D2D_WAVES = D2D_THREADS / 64;

// a record of the setters' input that cannot be a voxel: count < 1 or a non-finite sum
__global__ void __launch_bounds__(D2D_THREADS) k_d2d_check(const int32_t* __restrict__ count, const double* __restrict__ mom, int n,
                                                          int* __restrict__ bad) {
  const int r = (int)(blockIdx.x * D2D_THREADS + threadIdx.x);
  if (r >= n) return;
  bool b = count[r] < 1;
#pragma unroll
  for (int a = 0; a < 9; ++a) b = b || !isfinite(mom[(size_t)r * 9 + a]);
  if (b) atomicOr(bad, 1);
}

// record r -> a leaf through the target build's rule (cell = slot = r: cell2leaf[r] = r marks an accepted record, the
// array is -1 before the launch); counts[block] = records the block accepted
__global__ void __launch_bounds__(D2D_THREADS) k_d2d_finalize(const int32_t* __restrict__ count, const double* __restrict__ mom, int n,
                                                             int min_pts, FinalizeParams fp, VoxelRecord* __restrict__ rec,
                                                             float4* __restrict__ cent, LeafStats* __restrict__ stats,
                                                             int* __restrict__ cell2leaf, unsigned int* __restrict__ counts) {
  __shared__ unsigned int s_w[D2D_WAVES];
  const int r = (int)(blockIdx.x * D2D_THREADS + threadIdx.x);
  bool ok = false;
  if (r < n) {
    const int cnt = count[r];
    if (cnt >= min_pts) ok = finalize_leaf(r, r, cnt, mom + (size_t)r * 9, fp, rec, cent, stats, cell2leaf);
  }
  compact_ballot(ok, s_w);
  __syncthreads();
  compact_block_count(s_w, counts);
}

__global__ void __launch_bounds__(D2D_THREADS) k_d2d_emit(const int* __restrict__ cell2leaf, const LeafStats* __restrict__ stats, int n,
                                                         const unsigned int* __restrict__ offsets, double* __restrict__ gauss,
                                                         int32_t* __restrict__ gcount, int32_t* __restrict__ gindex) {
  __shared__ unsigned int s_w[D2D_WAVES];
  const int r = (int)(blockIdx.x * D2D_THREADS + threadIdx.x);
  const bool keep = r < n && cell2leaf[r] >= 0;
  const unsigned long long bal = compact_ballot(keep, s_w);
  __syncthreads();
  const unsigned int pos = compact_position(bal, s_w, offsets);
  if (!keep) return;   // (pos <= r < n: the outputs hold n Gaussians)
  const LeafStats& L = stats[r];
  double* g = gauss + (size_t)pos * 9;
  g[0] = L.mean[0]; g[1] = L.mean[1]; g[2] = L.mean[2];
  g[3] = L.cov[0]; g[4] = L.cov[1]; g[5] = L.cov[2]; g[6] = L.cov[4]; g[7] = L.cov[5]; g[8] = L.cov[8];
  gcount[pos] = L.count;
  gindex[pos] = r;
}

// leaf slot s of the target -> {mean 3, cov xx xy xz yy yz zz}: 72 bytes per pair in place of a 296-byte LeafStats
__global__ void __launch_bounds__(D2D_THREADS) k_d2d_gather_target(const LeafStats* __restrict__ stats, int n_slots,
                                                                  double* __restrict__ tleaf) {
  const int s = (int)(blockIdx.x * D2D_THREADS + threadIdx.x);
  if (s >= n_slots) return;
  const LeafStats& L = stats[s];
  double* g = tleaf + (size_t)s * 9;
  g[0] = L.mean[0]; g[1] = L.mean[1]; g[2] = L.mean[2];
  g[3] = L.cov[0]; g[4] = L.cov[1]; g[5] = L.cov[2]; g[6] = L.cov[4]; g[7] = L.cov[5]; g[8] = L.cov[8];
}

// One source Gaussian per lane: the moved mean, the neighbours of the f32-rounded moved mean (neighbor_cells7: DIRECT1 /
// DIRECT7, the pair order of every evaluator), the pairs, and the block's row of EV_WORDS sums (word 31 = 0).
template <bool HESSIAN, bool D7>
__global__ void __launch_bounds__(D2D_THREADS)
k_d2d_eval(const double* __restrict__ gauss, int n, GridGeom g, const int* __restrict__ cell2leaf, const double* __restrict__ tleaf,
           D2dPose P, double d1, double d2, double* __restrict__ rows) {
  __shared__ double s_part[D2D_WAVES][EV_WORDS];
  const int i = (int)(blockIdx.x * D2D_THREADS + threadIdx.x);
  const bool active = i < n;
  D2dAcc<HESSIAN> acc;
  acc.score = 0.0; acc.best = 0.0; acc.npairs = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) acc.g[a] = 0.0;
#pragma unroll
  for (int a = 0; a < (HESSIAN ? 21 : 1); ++a) acc.H[a] = 0.0;
  acc.w[0] = acc.w[1] = acc.w[2] = 0.0;
  acc.W.xx = acc.W.xy = acc.W.xz = acc.W.yy = acc.W.yz = acc.W.zz = 0.0;
  if (active) {
    const double* G = gauss + (size_t)i * 9;
    const double mu[3] = {G[0], G[1], G[2]};
    Sym3 S;
    S.xx = G[3]; S.xy = G[4]; S.xz = G[5]; S.yy = G[6]; S.yz = G[7]; S.zz = G[8];
    double m[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = ((P.R[3 * a] * mu[0] + P.R[3 * a + 1] * mu[1]) + P.R[3 * a + 2] * mu[2]) + P.t[a];
    const float xt = (float)m[0], yt = (float)m[1], zt = (float)m[2];
    const bool finite = isfinite(xt) && isfinite(yt) && isfinite(zt);
    int cell[7], slot[7];
    neighbor_cells7<D7>(xt, yt, zt, g, cell);
    neighbor_slots7<D7>(cell, finite, cell2leaf, slot);
    bool any = false;
#pragma unroll
    for (int k = 0; k < (D7 ? 7 : 1); ++k) any = any || slot[k] >= 0;
    if (any) {
      // what depends on the pose and the source Gaussian alone, once per lane
      double M[9];
      a_s_bt(P.R, S, P.R, M);
      Sym3 A;
      A.xx = M[0]; A.xy = M[1]; A.xz = M[2]; A.yy = M[4]; A.yz = M[5]; A.zz = M[8];
      double j[3][3];
      Sym3 Z[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        mat_vec(P.dR[c], mu, j[c]);
        a_s_bt(P.dR[c], S, P.R, M);
        Z[c] = sym_of(M);
      }
      const D2dNdtWeight wt{d1, d2};
#pragma unroll
      for (int k = 0; k < (D7 ? 7 : 1); ++k)
        if (slot[k] >= 0) d2d_pair<HESSIAN>(acc, tleaf + (size_t)slot[k] * 9, m, A, j, Z, wt);
      if (HESSIAN && acc.npairs > 0) {
        // the rotation block's second-derivative terms: 2 w^T H_cd - <Z_cd, W>, Z_cd = N + N^T,
        // N = (d2R_cd) S R^T + (dR_c) S (dR_d)^T
        int q = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int d = c; d < 3; ++d) {
            double hcd[3], N[9], N2[9];
            mat_vec(P.d2R[q], mu, hcd);
            a_s_bt(P.d2R[q], S, P.R, N);
            a_s_bt(P.dR[c], S, P.dR[d], N2);
#pragma unroll
            for (int a = 0; a < 9; ++a) N[a] += N2[a];
            const Sym3 Zcd = sym_of(N);
            // word of (3 + c, 3 + d) in the upper triangle row by row: rows 0 .. 2 hold 6 + 5 + 4 = 15 words
            const int word = 15 + (c == 0 ? d : c == 1 ? 3 + (d - 1) : 5);
            acc.H[word] += 2.0 * dot3(acc.w, hcd) - sym_inner(Zcd, acc.W);
            ++q;
          }
      }
    }
  }
  // lane -> wave -> block
  double words[EV_WORDS];
  words[EV_SCORE] = acc.score;
#pragma unroll
  for (int a = 0; a < 6; ++a) words[EV_G + a] = acc.g[a];
#pragma unroll
  for (int a = 0; a < 21; ++a) words[EV_H + a] = HESSIAN ? acc.H[a] : 0.0;
  words[EV_NVTL] = acc.best;
  words[EV_NWITH] = acc.npairs > 0 ? 1.0 : 0.0;
  words[EV_NPAIRS] = (double)acc.npairs;
  words[EV_FAIL] = 0.0;
  eval_block_row<D2D_WAVES, HESSIAN>(words, s_part, rows);
}

int blocks_for(size_t n) { return (int)((n + D2D_THREADS - 1) / D2D_THREADS); }

}  // namespace

namespace engine {
namespace {

int d2d_min_points(const ndt_handle* h) { return std::max(3, h->prm.min_points_per_voxel); }   // the ordinary build's rule (build_begin)

// the kept records -> the accepted Gaussians under the handle's leaf rule, in input order; awaited
int d2d_derive(ndt_handle* h) {
  D2dBufs& d = h->d2d;
  const size_t n = d.n_records;
  const int nb = blocks_for(n);
  HIP_TRY(h, d.frec.ensure(n));
  HIP_TRY(h, d.fcent.ensure(4 * n));
  HIP_TRY(h, d.fstats.ensure(n));
  HIP_TRY(h, d.fcell.ensure(n));
  HIP_TRY(h, d.gauss.ensure(9 * n));
  HIP_TRY(h, d.gcount.ensure(n));
  HIP_TRY(h, d.gindex.ensure(n));
  if (int rc = compact_scratch(h, nb)) return rc;
  hipStream_t s = h->stream;
  const int min_pts = d2d_min_points(h);
  const FinalizeParams fp{h->prm.eig_inflation_ratio, h->prm.cov_mode};
  HIP_TRY(h, hipMemsetAsync(d.fcell.p, 0xff, n * sizeof(int), s));
  unsigned int* counts = h->compact.counts.p;
  hipLaunchKernelGGL(k_d2d_finalize, dim3((unsigned)nb), dim3(D2D_THREADS), 0, s, d.rcount.p, d.rmom.p, (int)n, min_pts, fp, d.frec.p,
                     reinterpret_cast<float4*>(d.fcent.p), d.fstats.p, d.fcell.p, counts);
  launch_filter_scan(counts, nb, h->compact.d_total(nb), s);
  hipLaunchKernelGGL(k_d2d_emit, dim3((unsigned)nb), dim3(D2D_THREADS), 0, s, d.fcell.p, d.fstats.p, (int)n, counts, d.gauss.p,
                     d.gcount.p, d.gindex.p);
  size_t kept = 0;
  if (int rc = compact_total(h, nb, n, &kept)) return rc;
  d.n_accepted = kept;
  d.rule_min_pts = min_pts;
  d.rule_cov_mode = h->prm.cov_mode;
  d.rule_eig = h->prm.eig_inflation_ratio;
  return NDT_OK;
}

// the Gaussians follow the handle's leaf rule: ndt_set_params may have changed it since they were derived
int d2d_source_fresh(ndt_handle* h) {
  const D2dBufs& d = h->d2d;
  if (!d.have || d.n_records == 0) return NDT_OK;
  if (d.rule_min_pts == d2d_min_points(h) && d.rule_cov_mode == h->prm.cov_mode && d.rule_eig == h->prm.eig_inflation_ratio)
    return NDT_OK;
  return d2d_derive(h);
}

void d2d_clear(ndt_handle* h) {
  h->d2d.have = false;
  h->d2d.n_records = h->d2d.n_accepted = 0;
}

bool d2d_too_many(size_t n) { return n > (size_t)std::numeric_limits<int>::max() / 16; }

// target, then distribution source: what ndt_align_d2d answers with the guess
int d2d_ready(ndt_handle* h) {
  if (int rc = settle(h)) return rc;
  if (int rc = lane_eval_supported(h, "D2D")) return rc;
  if (int rc = d2d_source_fresh(h)) return rc;
  if (!h->d2d.have || h->d2d.n_accepted == 0)
    return fail(h, NDT_ERR_NO_SOURCE, "no source Gaussians (ndt_set_source_distributions first)");
  D2dBufs& d = h->d2d;
  if (!d.tleaf_valid || d.tleaf_gen != h->tgt.gen()) {
    const int n_slots = h->tgt.n_slots();
    HIP_TRY(h, d.tleaf.ensure(9 * (size_t)n_slots));
    hipLaunchKernelGGL(k_d2d_gather_target, dim3((unsigned)blocks_for((size_t)n_slots)), dim3(D2D_THREADS), 0, h->stream, h->stats.p,
                       n_slots, d.tleaf.p);
    HIP_TRY(h, hipGetLastError());
    d.tleaf_gen = h->tgt.gen();
    d.tleaf_valid = true;
  }
  return NDT_OK;
}

// K poses -> K x EV_WORDS raw sums in `out`; d2d_ready has passed
int d2d_eval_raw(ndt_handle* h, const double* poses6, int K, bool need_h, double* out) {
  D2dBufs& d = h->d2d;
  const int n = (int)d.n_accepted, nb = blocks_for(d.n_accepted);
  double d1, d2;
  gauss_constants((double)h->prm.resolution, h->prm.outlier_ratio, &d1, &d2);
  const bool d7 = h->prm.search_method == NDT_DIRECT7;
  const dim3 grid((unsigned)nb), block(D2D_THREADS);
  return lane_eval_rows(h, "D2D", nb, K, [&](int k, double* rows) {
    D2dPose P;
    fill_d2d_pose(poses6 + 6 * (size_t)k, &P);
#define NDT_D2D_LAUNCH(H, D7) \
  hipLaunchKernelGGL((k_d2d_eval<H, D7>), grid, block, 0, h->stream, d.gauss.p, n, h->geom, h->cell2leaf.p, d.tleaf.p, P, d1, d2, rows)
    if (need_h) { if (d7) NDT_D2D_LAUNCH(true, true); else NDT_D2D_LAUNCH(true, false); }
    else { if (d7) NDT_D2D_LAUNCH(false, true); else NDT_D2D_LAUNCH(false, false); }
#undef NDT_D2D_LAUNCH
  }, out);
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

int ndt_set_source_distributions(ndt_handle* h, const int32_t* count, const double* moments9, size_t n) {
  if (!h || (n && (!count || !moments9)) || d2d_too_many(n)) return NDT_ERR_INVALID_ARG;
  for (size_t r = 0; r < n; ++r) {   // (before the handle is looked at: a refused call leaves the previous source)
    if (count[r] < 1 || !all_finite(moments9 + 9 * r, 9)) return NDT_ERR_INVALID_ARG;
  }
  if (n == 0) { d2d_clear(h); return NDT_OK; }
  if (int rc = bind_device(h)) return rc;
  D2dBufs& d = h->d2d;
  HIP_TRY(h, d.rcount.ensure(n));
  HIP_TRY(h, d.rmom.ensure(9 * n));
  d2d_clear(h);   // (from here on the previous source is gone)
  HIP_TRY(h, hipMemcpyAsync(d.rcount.p, count, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(d.rmom.p, moments9, 9 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  d.n_records = n;
  if (int rc = d2d_derive(h)) { d2d_clear(h); return rc; }
  d.have = true;
  return NDT_OK;
}

int ndt_set_source_distributions_device(ndt_handle* h, const int32_t* d_count, const double* d_moments9, size_t n) {
  if (!h || (n && (!d_count || !d_moments9)) || d2d_too_many(n)) return NDT_ERR_INVALID_ARG;
  if (n == 0) { d2d_clear(h); return NDT_OK; }
  if (int rc = bind_device(h)) return rc;
  D2dBufs& d = h->d2d;
  HIP_TRY(h, d.bad.ensure(1));
  HIP_TRY(h, d.bad_h.ensure(4));
  hipStream_t s = h->stream;
  HIP_TRY(h, hipMemsetAsync(d.bad.p, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_d2d_check, dim3((unsigned)blocks_for(n)), dim3(D2D_THREADS), 0, s, d_count, d_moments9, (int)n, d.bad.p);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(d.bad_h.h, d.bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  if (d.bad_h.h[0]) return fail(h, NDT_ERR_INVALID_ARG, "source distributions: a count < 1 or a non-finite moment");
  if (d_count != d.rcount.p) {   // (the handle's own kept records may be handed back)
    HIP_TRY(h, d.rcount.ensure(n));
    HIP_TRY(h, d.rmom.ensure(9 * n));
    d2d_clear(h);
    HIP_TRY(h, hipMemcpyAsync(d.rcount.p, d_count, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(d.rmom.p, d_moments9, 9 * n * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  d.n_records = n;
  if (int rc = d2d_derive(h)) { d2d_clear(h); return rc; }
  d.have = true;
  return NDT_OK;
}

int ndt_source_distributions_info(ndt_handle* h, int64_t* n_records, int64_t* n_accepted) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (h->d2d.have) {
    if (int rc = bind_device(h)) return rc;
    if (int rc = d2d_source_fresh(h)) return rc;
  }
  if (n_records) *n_records = h->d2d.have ? (int64_t)h->d2d.n_records : 0;
  if (n_accepted) *n_accepted = h->d2d.have ? (int64_t)h->d2d.n_accepted : 0;
  return NDT_OK;
}

int64_t ndt_export_source_distributions(ndt_handle* h, double* mean3, double* cov6, int32_t* count, int32_t* record_index,
                                        size_t cap) {
  if (!h) return NDT_ERR_INVALID_ARG;
  const D2dBufs& d = h->d2d;
  if (!d.have) return 0;
  if (int rc = bind_device(h)) return rc;
  if (int rc = d2d_source_fresh(h)) return rc;
  const size_t m = d.n_accepted;
  if (m > cap) return over_capacity(h, m);
  if (m == 0) return 0;
  std::vector<double> g(9 * m);
  hipStream_t s = h->stream;
  HIP_TRY(h, hipMemcpyAsync(g.data(), d.gauss.p, 9 * m * sizeof(double), hipMemcpyDeviceToHost, s));
  if (count) HIP_TRY(h, hipMemcpyAsync(count, d.gcount.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (record_index) HIP_TRY(h, hipMemcpyAsync(record_index, d.gindex.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  for (size_t i = 0; i < m; ++i) {
    if (mean3) std::memcpy(mean3 + 3 * i, &g[9 * i], 3 * sizeof(double));
    if (cov6) std::memcpy(cov6 + 6 * i, &g[9 * i + 3], 6 * sizeof(double));
  }
  return (int64_t)m;
}

int ndt_eval_derivatives_d2d(ndt_handle* h, const double* poses6, int K, int compute_hessian, double* out) {
  if (!h || !poses6 || !out || K <= 0) return NDT_ERR_INVALID_ARG;
  if (!all_finite(poses6, 6 * (size_t)K)) return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = d2d_ready(h)) return rc;
  if (int rc = d2d_eval_raw(h, poses6, K, compute_hessian != 0, out)) return rc;
  for (int k = 0; k < K; ++k) finish_words(h, poses6 + 6 * (size_t)k, compute_hessian != 0, out + (size_t)k * EV_WORDS);
  return NDT_OK;
}

int ndt_align_d2d(ndt_handle* h, const float guess[16], ndt_result* out) {
  if (!h || !guess || !out) return NDT_ERR_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));   // what every failure before the loop leaves: the guess, not converged
  std::memcpy(out->final_transformation, guess, sizeof(float) * 16);
  if (int rc = bind_device(h)) return rc;
  h->keepwarm.touch();
  if (int rc = d2d_ready(h)) return rc;
  return lane_align(h, (int64_t)h->d2d.n_accepted, guess,
                    [h](const double* p, bool need_h, double* words) { return d2d_eval_raw(h, p, 1, need_h, words); }, out);
}

}  // extern "C"
