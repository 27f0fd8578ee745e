// ndt_vgicp.hip -- voxelised GICP (Koide et al. 2021): GICP's plane-to-plane cost with one aggregate per target voxel as
// the partner instead of the nearest target point (see ndt_engine.h; the rule is stated in include/ndt_hip.h):
//   table        k_vgicp_keys -- one lane per target point: the leaf slot its f32 classification (neighbor_cells7<false>)
//                gives it, or the sentinel n_slots for a point that is not finite, has no covariance or lies in no leaf;
//                the stable keyed sort by slot (sort_keyed, ndt_sort.hip); k_vgicp_voxels -- one lane per leaf slot walks
//                its run of the sorted pairs in input order: two in-order f64 sums (points, covariances) and the divisions
//   evaluation   k_vgicp_eval<HESSIAN, D7> -- one source point per lane, the voxels of its moved point by the shared
//                neighbour rule (ndt_neighbors_device.h), up to seven d2d_pair calls with the weight -N / 2
//                (D2dCountWeight, ndt_d2d_device.h); rows, fixed-order sum and align are ndt_eval_rows.hip's
// The point covariances of both clouds are GICP's (ndt_gicp.hip: h->gicp.tgt / h->gicp.src).  The handle's align state,
// iteration history, point source, distribution source and frozen GICP pairs are not touched.
#include "ndt_engine.h"
#include "ndt_d2d_device.h"
#include "ndt_evalrows_device.h"
#include "ndt_neighbors_device.h"

namespace ndt {
namespace engine {
namespace {

constexpr int VGICP_THREADS = 256, VGICP_WAVES = VGICP_THREADS / 64;
constexpr int VGICP_MIN_NEIGHBOURS = 4;   // GICP's: a point with fewer neighbours has no covariance

// target point i -> the slot of the leaf it was built into, or n_slots
__global__ void __launch_bounds__(VGICP_THREADS)
k_vgicp_keys(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, const int32_t* __restrict__ nfound,
             int n, GridGeom g, const int* __restrict__ cell2leaf, int n_slots, uint32_t* __restrict__ keys) {
  const int i = (int)(blockIdx.x * VGICP_THREADS + threadIdx.x);
  if (i >= n) return;
  const float px = x[i], py = y[i], pz = z[i];
  int slot = -1;
  if (isfinite(px) && isfinite(py) && isfinite(pz) && nfound[i] >= VGICP_MIN_NEIGHBOURS) {
    int cell[7];
    neighbor_cells7<false>(px, py, pz, g, cell);   // (cell[0] is -1 or inside [0, ncells))
    if (cell[0] >= 0) slot = cell2leaf[cell[0]];
  }
  keys[i] = (slot >= 0 && slot < n_slots) ? (uint32_t)slot : (uint32_t)n_slots;
}

// leaf slot l: its run of the n sorted (slot, point) pairs, in input order
__global__ void __launch_bounds__(VGICP_THREADS)
k_vgicp_voxels(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, int n, const double* __restrict__ tgauss,
               int n_slots, double* __restrict__ table, int32_t* __restrict__ count) {
  const int l = (int)(blockIdx.x * VGICP_THREADS + threadIdx.x);
  if (l >= n_slots) return;
  int lo = 0, hi = n;   // the first pair whose key is >= l
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (keys[mid] < (uint32_t)l) lo = mid + 1; else hi = mid;
  }
  double s[3] = {0.0, 0.0, 0.0}, c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int m = 0;
  for (int r = lo; r < n && keys[r] == (uint32_t)l; ++r) {
    const double* G = tgauss + (size_t)vals[r] * 9;   // {the point as f64, its regularised covariance}
#pragma unroll
    for (int a = 0; a < 3; ++a) s[a] += G[a];
#pragma unroll
    for (int a = 0; a < 6; ++a) c[a] += G[3 + a];
    ++m;
  }
  double* T = table + (size_t)l * 9;
  const double dm = (double)m;
#pragma unroll
  for (int a = 0; a < 3; ++a) T[a] = m > 0 ? s[a] / dm : NAN;
#pragma unroll
  for (int a = 0; a < 6; ++a) T[3 + a] = m > 0 ? c[a] / dm : NAN;
  count[l] = m;
}

// One source point per lane: the voxels of its moved point through d2d_pair with the weight -N / 2, and the block's row
// of EV_WORDS sums (nvtl_sum = score; word 31 = 0).
template <bool HESSIAN, bool D7>
__global__ void __launch_bounds__(VGICP_THREADS)
k_vgicp_eval(const double* __restrict__ sgauss, int n, GridGeom g, const int* __restrict__ cell2leaf, const double* __restrict__ table,
             const int32_t* __restrict__ count, D2dPose P, double* __restrict__ rows) {
  __shared__ double s_part[VGICP_WAVES][EV_WORDS];
  const int i = (int)(blockIdx.x * VGICP_THREADS + threadIdx.x);
  D2dAcc<HESSIAN> acc;
  d2d_acc_clear(acc);
  if (i < n) {
    const double* G = sgauss + (size_t)i * 9;
    const double mu[3] = {G[0], G[1], G[2]};
    Sym3 S;
    S.xx = G[3]; S.xy = G[4]; S.xz = G[5]; S.yy = G[6]; S.yz = G[7]; S.zz = G[8];
    double m[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = ((P.R[3 * a] * mu[0] + P.R[3 * a + 1] * mu[1]) + P.R[3 * a + 2] * mu[2]) + P.t[a];
    const float xt = (float)m[0], yt = (float)m[1], zt = (float)m[2];
    // (a point without a covariance carries NaN there)
    const bool finite = !isnan(S.xx) && isfinite(xt) && isfinite(yt) && isfinite(zt);
    int cell[7], slot[7];
    neighbor_cells7<D7>(xt, yt, zt, g, cell);
    neighbor_slots7<D7>(cell, finite, cell2leaf, slot);
    bool any = false;
#pragma unroll
    for (int k = 0; k < (D7 ? 7 : 1); ++k) any = any || slot[k] >= 0;
    if (any) {
      // what depends on the pose and the source point alone, once per lane.  Written out as k_d2d_eval has it, not through
      // d2d_source_terms / d2d_second_order: with those the <true, true> instance needs 255 VGPRs and 34 AGPRs
      double M[9];
      a_s_bt(P.R, S, P.R, M);
      Sym3 A;
      A.xx = M[0]; A.xy = M[1]; A.xz = M[2]; A.yy = M[4]; A.yz = M[5]; A.zz = M[8];
      double jc[3][3];
      Sym3 Z[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        mat_vec(P.dR[c], mu, jc[c]);
        a_s_bt(P.dR[c], S, P.R, M);
        Z[c] = sym_of(M);
      }
#pragma unroll
      for (int k = 0; k < (D7 ? 7 : 1); ++k) {
        const int cnt = slot[k] >= 0 ? count[slot[k]] : 0;   // (a leaf none of whose points contributes: N = 0, no pair)
        if (cnt > 0) d2d_pair<HESSIAN>(acc, table + (size_t)slot[k] * 9, m, A, jc, Z, D2dCountWeight{(double)cnt});
      }
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
            const int word = 15 + (c == 0 ? d : c == 1 ? 3 + (d - 1) : 5);
            acc.H[word] += 2.0 * dot3(acc.w, hcd) - sym_inner(Zcd, acc.W);
            ++q;
          }
      }
    }
  }
  double words[EV_WORDS];
  d2d_words(acc, acc.score, words);
  eval_block_row<VGICP_WAVES, HESSIAN>(words, s_part, rows);
}

unsigned blocks_of(size_t n) { return (unsigned)((n + VGICP_THREADS - 1) / VGICP_THREADS); }

// the table of the published target, fresh; the target's covariances are ready
int vgicp_derive(ndt_handle* h) {
  VgicpBufs& v = h->vgicp;
  const GicpCloud& c = h->gicp.tgt;
  v.valid = false;
  const size_t n = c.n;
  const int n_slots = h->tgt.n_slots();
  HIP_TRY(h, v.table.ensure(9 * (size_t)n_slots));
  HIP_TRY(h, v.count.ensure((size_t)n_slots));
  HIP_TRY(h, v.sort.ensure(n));
  HIP_TRY(h, v.plan.ensure(1));
  hipStream_t s = h->stream;
  hipLaunchKernelGGL(k_vgicp_keys, dim3(blocks_of(n)), dim3(VGICP_THREADS), 0, s, h->tx.p, h->ty.p, h->tz.p, c.nfound.p, (int)n, h->geom,
                     h->cell2leaf.p, n_slots, v.sort.keys.p);
  int passes = 0;
  if (int rc = sort_put_plan(h, v.plan.p, sort_key_bits(n_slots), 0, &passes)) return rc;   // (the last key is n_slots)
  SortedPairs sorted;
  HIP_TRY(h, sort_keyed(v.sort, n, v.plan.p, passes, SORT_COUNT_FIRST, s, &sorted));
  hipLaunchKernelGGL(k_vgicp_voxels, dim3(blocks_of((size_t)n_slots)), dim3(VGICP_THREADS), 0, s, sorted.keys, sorted.vals, (int)n,
                     c.gauss.p, n_slots, v.table.p, v.count.p);
  HIP_TRY(h, hipGetLastError());
  std::vector<int32_t> cnt((size_t)n_slots);
  HIP_TRY(h, hipMemcpyAsync(cnt.data(), v.count.p, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  v.n_voxels = v.n_points = 0;
  for (int32_t m : cnt) {
    v.n_voxels += m > 0 ? 1 : 0;
    v.n_points += m;
  }
  v.n_slots = n_slots;
  v.gen = h->tgt.gen();
  v.valid = true;
  return NDT_OK;
}

// what every VGICP call checks first, then the target's covariances and the table
int vgicp_target_ready(ndt_handle* h) {
  if (int rc = gicp_settle(h)) return rc;
  if (int rc = gicp_target_state(h)) return rc;
  if (int rc = lane_eval_supported(h, "VGICP")) return rc;
  if (int rc = gicp_target_ready(h)) return rc;
  const VgicpBufs& v = h->vgicp;
  if (v.valid && v.gen == h->tgt.gen()) return NDT_OK;
  return vgicp_derive(h);
}

int vgicp_ready(ndt_handle* h) {
  if (int rc = vgicp_target_ready(h)) return rc;
  if (int rc = gicp_source_ready(h)) return rc;
  if (h->gicp.src.n_without >= (int64_t)h->gicp.src.n)
    return fail(h, NDT_ERR_NO_SOURCE, "VGICP: no source point has a covariance");
  return NDT_OK;
}

// K poses -> K x EV_WORDS raw sums in `out`; vgicp_ready has passed
int vgicp_eval_raw(ndt_handle* h, const double* poses6, int K, bool need_h, double* out) {
  const GicpCloud& src = h->gicp.src;
  const VgicpBufs& v = h->vgicp;
  const int n = (int)src.n, nb = (int)blocks_of(src.n);
  const bool d7 = h->prm.search_method == NDT_DIRECT7;
  const dim3 grid((unsigned)nb), block(VGICP_THREADS);
  return lane_eval_rows(h, "VGICP", nb, K, [&](int k, double* rows) {
    D2dPose P;
    fill_d2d_pose(poses6 + 6 * (size_t)k, &P);
#define NDT_VGICP_LAUNCH(H, D7) \
  hipLaunchKernelGGL((k_vgicp_eval<H, D7>), grid, block, 0, h->stream, src.gauss.p, n, h->geom, h->cell2leaf.p, v.table.p, v.count.p, P, rows)
    if (need_h) { if (d7) NDT_VGICP_LAUNCH(true, true); else NDT_VGICP_LAUNCH(true, false); }
    else { if (d7) NDT_VGICP_LAUNCH(false, true); else NDT_VGICP_LAUNCH(false, false); }
#undef NDT_VGICP_LAUNCH
  }, out);
}

void vgicp_fill_info(const ndt_handle* h, ndt_vgicp_info* info) {
  std::memset(info, 0, sizeof(*info));
  info->n_voxels = h->vgicp.n_voxels;
  info->n_leaves = h->tgt.n_valid();
  info->n_target_points_in_voxels = h->vgicp.n_points;
  info->n_target_without_covariance = h->gicp.tgt.n_without;
  info->n_source_without_covariance = h->gicp.src.valid ? h->gicp.src.n_without : 0;
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

int64_t ndt_vgicp_export_voxels(ndt_handle* h, int32_t* count, double* mean3, double* cov6, size_t cap) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = vgicp_target_ready(h)) return rc;
  const VgicpBufs& v = h->vgicp;
  const size_t n_slots = (size_t)v.n_slots;
  // the rows of ndt_export_leaves: the accepted leaves by ascending cell
  std::vector<LeafStats> st(n_slots);
  std::vector<double> tab(9 * n_slots);
  std::vector<int32_t> cnt(n_slots);
  if (n_slots) {
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(st.data(), h->stats.p, n_slots * sizeof(LeafStats), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(tab.data(), v.table.p, tab.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(cnt.data(), v.count.p, n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
  }
  std::vector<size_t> ok;
  ok.reserve(n_slots);
  for (size_t l = 0; l < n_slots; ++l)
    if (st[l].count > 0) ok.push_back(l);
  std::stable_sort(ok.begin(), ok.end(), [&st](size_t a, size_t b) { return st[a].cell < st[b].cell; });
  if (ok.size() > cap) return over_capacity(h, ok.size());
  for (size_t r = 0; r < ok.size(); ++r) {
    const size_t l = ok[r];
    if (count) count[r] = cnt[l];
    if (mean3) std::memcpy(mean3 + 3 * r, &tab[9 * l], 3 * sizeof(double));
    if (cov6) std::memcpy(cov6 + 6 * r, &tab[9 * l + 3], 6 * sizeof(double));
  }
  return (int64_t)ok.size();
}

int ndt_vgicp_get_info(ndt_handle* h, ndt_vgicp_info* out) {
  if (!h || !out) return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = vgicp_target_ready(h)) return rc;
  if (h->n_src != 0 && h->vx)
    if (int rc = gicp_source_ready(h)) return rc;
  vgicp_fill_info(h, out);
  return NDT_OK;
}

int ndt_eval_derivatives_vgicp(ndt_handle* h, const double* poses6, int K, int compute_hessian, double* out) {
  if (!h || !poses6 || !out || K <= 0) return NDT_ERR_INVALID_ARG;
  for (int k = 0; k < K; ++k)
    if (!all_finite(poses6 + 6 * (size_t)k, 6)) return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = vgicp_ready(h)) return rc;
  if (int rc = vgicp_eval_raw(h, poses6, K, compute_hessian != 0, out)) return rc;
  for (int k = 0; k < K; ++k) finish_words(h, poses6 + 6 * (size_t)k, compute_hessian != 0, out + (size_t)k * EV_WORDS);
  return NDT_OK;
}

int ndt_align_vgicp(ndt_handle* h, const float guess[16], ndt_result* out, ndt_vgicp_info* info) {
  if (!h || !guess || !out) return NDT_ERR_INVALID_ARG;
  const auto give_guess = [&]() {   // what every failure leaves: the guess, not converged
    std::memset(out, 0, sizeof(*out));
    std::memcpy(out->final_transformation, guess, sizeof(float) * 16);
  };
  give_guess();
  if (info) std::memset(info, 0, sizeof(*info));
  if (int rc = bind_device(h)) return rc;
  h->keepwarm.touch();
  if (int rc = vgicp_ready(h)) return rc;
  double p[6];
  matrix_to_pose(guess, p);
  if (!all_finite(p, 6)) return fail(h, NDT_ERR_INVALID_ARG, "VGICP: the guess is not a finite pose");
  double last_pairs = 0.0, last_with = 0.0;
  const int rc = lane_align(h, (int64_t)h->n_src, guess, [&](const double* q, bool need_h, double* words) {
    const int r = vgicp_eval_raw(h, q, 1, need_h, words);
    if (r == NDT_OK) { last_pairs = words[EV_NPAIRS]; last_with = words[EV_NWITH]; }
    return r;
  }, out);
  if (rc) { give_guess(); return rc; }
  if (info) {
    vgicp_fill_info(h, info);
    info->n_pairs = (int64_t)last_pairs;
    info->n_source_with_pairs = (int64_t)last_with;
  }
  return NDT_OK;
}

}  // extern "C"
