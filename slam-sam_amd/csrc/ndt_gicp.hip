// ndt_gicp.hip -- generalised ICP (Segal et al. 2009) in PCL's plane-to-plane form (see ndt_engine.h; the rule is stated
// in include/ndt_hip.h):
//   neighbours   k_gicp_knn<KMAX> / k_gicp_knn_tail<KMAX> -- one lane per point over the cloud's point index (the fitness
//                index: ndt_fit_device.h): pass 1 scans the 27 cells around the point, the points it cannot settle there are
//                queued and pass 2 walks Chebyshev shells until the k-th best d^2 is at or below the conservative lower
//                bound on everything unscanned (fit_lower_bound2).  The lane's top-k list lives in registers: KMAX
//                (d2, index) pairs that are only ever indexed by unrolled compile-time indices (an insertion is one
//                compare-swap chain), KMAX = 8 / 16 / 24 / 32 by k_neighbours.  Blocks are ONE wave: a 4 500-point scan
//                then spreads over 71 compute units instead of 18, and a lane that walks far holds up 63 others, not 255.
//   covariances  k_gicp_cov -- the neighbour list's mean and covariance in two in-order f64 passes, the normal by the
//                target build's Jacobi rotations (jacobi_rot, ndt_leaf_device.h), C = I - (1 - eps) n n^T
//   pairing      k_gicp_pair / k_gicp_pair_tail -- the nearest target point by (d2, input index), the same two passes
//   evaluation   k_gicp_eval<HESSIAN> -- one source point per lane over the frozen pairs through d2d_pair
//                (ndt_d2d_device.h) with the weight -1/2; rows, fixed-order sum and align are ndt_eval_rows.hip's
// The handle's align state, iteration history, point source and distribution source are not touched.
#include "ndt_engine.h"
#include "ndt_d2d_device.h"
#include "ndt_evalrows_device.h"
#include "ndt_fit_device.h"
#include "ndt_leaf_device.h"

namespace ndt {
namespace engine {
namespace {

constexpr int KNN_THREADS = 64;                      // one wave per block (see above)
constexpr int GICP_THREADS = 256, GICP_WAVES = GICP_THREADS / 64;
constexpr int GICP_TAIL_BLOCKS = 1024;               // pass 2: grid-stride over the queued points
constexpr int GICP_MIN_NEIGHBOURS = 4;
// words of GicpBufs::work in front of the queue
constexpr int W_QUEUED = 0, W_WITHOUT = 1, W_PAIRS = 2, W_QUEUE = 4;

// (d, i) before (e, j) in the order of the rule
__device__ __forceinline__ bool gicp_before(float d, int i, float e, int j) { return d < e || (d == e && i < j); }

// a search has settled after the box of radius r: nothing unscanned can come before the k-th best (lb2 == 0 says nothing:
// the query sits on the face within the bound's slack), or nothing unscanned lies within the cap
__device__ __forceinline__ bool gicp_settled(float kth, float lb2, float cap2) { return (kth <= lb2 && lb2 > 0.0f) || lb2 > cap2; }

// The exact k nearest neighbours of point i of the indexed cloud, scanning boxes up to radius r_limit.  false: not settled
// within r_limit (nothing is written).
template <int KMAX>
__device__ __forceinline__ bool gicp_knn_point(float px, float py, float pz, int i, const FitGeom& g, const float4* __restrict__ pts,
                                               const uint4* __restrict__ tab, int k, float cap2, int r_limit,
                                               int32_t* __restrict__ nbr, int32_t* __restrict__ nfound) {
  float d[KMAX];
  int id[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) { d[j] = INFINITY; id[j] = INT_MAX; }
  float kth_d = INFINITY;
  int kth_i = INT_MAX;
  const int km1 = k - 1;
  FitQuery q;
  q.qx = px; q.qy = py; q.qz = pz;
  fit_locate(g, &q);
  auto scan = [&](int cx, int cy, int cz) __attribute__((always_inline)) {
    uint32_t first, end;
    if (!fit_find(tab, g.hash_mask, fit_key(g, cx, cy, cz), &first, &end)) return;
    for (uint32_t s = first; s < end; ++s) {
      const float4 p = pts[s];
      const float dx = p.x - q.qx, dy = p.y - q.qy, dz = p.z - q.qz;
      float cd = (dx * dx + dy * dy) + dz * dz;
      int ci = __float_as_int(p.w);
      if (cd > cap2 || !gicp_before(cd, ci, kth_d, kth_i)) continue;
      // one compare-swap chain: the candidate sinks to its place, what it displaces moves on
#pragma unroll
      for (int j = 0; j < KMAX; ++j) {
        const bool in = gicp_before(cd, ci, d[j], id[j]);
        const float td = d[j];
        const int ti = id[j];
        d[j] = in ? cd : td; id[j] = in ? ci : ti;
        cd = in ? td : cd; ci = in ? ti : ci;
        if (j == km1) { kth_d = d[j]; kth_i = id[j]; }
      }
    }
  };
  fit_walk_box(q, g, scan);
  for (int r = 1;; ++r) {
    if (gicp_settled(kth_d, fit_lower_bound2(q, g, r), cap2)) break;
    if (r >= r_limit) return false;
    fit_walk_shell(q, g, r + 1, scan);
  }
  int m = 0;
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
    if (j < k) {
      const bool have = id[j] != INT_MAX;
      nbr[(size_t)i * k + j] = have ? id[j] : -1;
      m += have ? 1 : 0;
    }
  nfound[i] = m;
  return true;
}

// pass 1: one lane per point, the 27 cells around it; what does not settle there is queued
template <int KMAX>
__global__ void __launch_bounds__(KNN_THREADS)
k_gicp_knn(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n, FitGeom g,
           const float4* __restrict__ pts, const uint4* __restrict__ tab, int k, float cap2, int32_t* __restrict__ nbr,
           int32_t* __restrict__ nfound, int* __restrict__ work) {
  const int i = (int)(blockIdx.x * KNN_THREADS + threadIdx.x);
  if (i >= n) return;
  const float px = x[i], py = y[i], pz = z[i];
  if (!finite3(px, py, pz)) {
    for (int j = 0; j < k; ++j) nbr[(size_t)i * k + j] = -1;
    nfound[i] = 0;
    return;
  }
  if (gicp_knn_point<KMAX>(px, py, pz, i, g, pts, tab, k, cap2, 1, nbr, nfound)) return;
  work[W_QUEUE + atomicAdd(&work[W_QUEUED], 1)] = i;   // (at most n entries)
}

// pass 2: the queued points from the start, shells until they settle (the box that covers the grid settles everything)
template <int KMAX>
__global__ void __launch_bounds__(KNN_THREADS)
k_gicp_knn_tail(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, FitGeom g,
                const float4* __restrict__ pts, const uint4* __restrict__ tab, int k, float cap2, int32_t* __restrict__ nbr,
                int32_t* __restrict__ nfound, const int* __restrict__ work) {
  const int total = work[W_QUEUED];
  for (int w = (int)(blockIdx.x * KNN_THREADS + threadIdx.x); w < total; w += (int)(gridDim.x * KNN_THREADS)) {
    const int i = work[W_QUEUE + w];
    gicp_knn_point<KMAX>(x[i], y[i], z[i], i, g, pts, tab, k, cap2, fit_rmax(g), nbr, nfound);
  }
}

// one point per lane: mean and raw covariance of its neighbour list in list order, the normal, the regularised covariance
__global__ void __launch_bounds__(GICP_THREADS)
k_gicp_cov(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n, int k,
           const int32_t* __restrict__ nbr, const int32_t* __restrict__ nfound, double eps, double* __restrict__ mean3,
           double* __restrict__ raw6, double* __restrict__ gauss, int* __restrict__ work) {
  const int i = (int)(blockIdx.x * GICP_THREADS + threadIdx.x);
  if (i >= n) return;
  double* G = gauss + (size_t)i * 9;
  G[0] = (double)x[i]; G[1] = (double)y[i]; G[2] = (double)z[i];
  const int m = nfound[i];
  if (m < GICP_MIN_NEIGHBOURS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) mean3[(size_t)i * 3 + a] = NAN;
#pragma unroll
    for (int a = 0; a < 6; ++a) { raw6[(size_t)i * 6 + a] = NAN; G[3 + a] = NAN; }
    atomicAdd(&work[W_WITHOUT], 1);
    return;
  }
  const int32_t* row = nbr + (size_t)i * k;
  double s[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < m; ++j) {
    const int p = row[j];
    s[0] += (double)x[p]; s[1] += (double)y[p]; s[2] += (double)z[p];
  }
  const double dm = (double)m;
  const double mean[3] = {s[0] / dm, s[1] / dm, s[2] / dm};
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < m; ++j) {
    const int p = row[j];
    const double dx = (double)x[p] - mean[0], dy = (double)y[p] - mean[1], dz = (double)z[p] - mean[2];
    c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz; c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) c[a] = c[a] / dm;
#pragma unroll
  for (int a = 0; a < 3; ++a) mean3[(size_t)i * 3 + a] = mean[a];
#pragma unroll
  for (int a = 0; a < 6; ++a) raw6[(size_t)i * 6 + a] = c[a];
  // the leaf rule's eigen-solver: cyclic Jacobi sweeps in f64 (finalize_leaf's loop over jacobi_rot), columns ascending
  double A[9] = {c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]}, V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
    double diag = A[0] * A[0] + A[4] * A[4] + A[8] * A[8];
    if (off <= 1e-32 * diag || off == 0.0) break;
    jacobi_rot<0, 1>(A, V);
    jacobi_rot<0, 2>(A, V);
    jacobi_rot<1, 2>(A, V);
  }
  double d[3] = {A[0], A[4], A[8]};
  if (d[0] > d[1]) NDT_SWAP_COL(0, 1);
  if (d[1] > d[2]) NDT_SWAP_COL(1, 2);
  if (d[0] > d[1]) NDT_SWAP_COL(0, 1);
  const double nx = V[0], ny = V[3], nz = V[6];
  const double w = 1.0 - eps;
  G[3] = 1.0 - (w * nx) * nx; G[4] = 0.0 - (w * nx) * ny; G[5] = 0.0 - (w * nx) * nz;
  G[6] = 1.0 - (w * ny) * ny; G[7] = 0.0 - (w * ny) * nz; G[8] = 1.0 - (w * nz) * nz;
}

struct GicpMove {
  double R[9], t[3];
};

// The nearest indexed point of source point i's moved position by (d2, input index), scanning boxes up to radius r_limit.
// false: not settled within r_limit (nothing is written).
__device__ __forceinline__ bool gicp_pair_point(int i, const double* __restrict__ sgauss, const GicpMove& P, const FitGeom& g,
                                                const float4* __restrict__ pts, const uint4* __restrict__ tab,
                                                const int32_t* __restrict__ tfound, float cap2, int r_limit,
                                                int32_t* __restrict__ pair, float* __restrict__ pd2, int* __restrict__ work) {
  const double* S = sgauss + (size_t)i * 9;
  int bi = INT_MAX;
  float bd = INFINITY;
  bool live = !isnan(S[3]);   // (a point without a covariance carries NaN there)
  FitQuery q;
  if (live) {
    double m[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = ((P.R[3 * a] * S[0] + P.R[3 * a + 1] * S[1]) + P.R[3 * a + 2] * S[2]) + P.t[a];
    q.qx = (float)m[0]; q.qy = (float)m[1]; q.qz = (float)m[2];
    live = finite3(q.qx, q.qy, q.qz);
  }
  if (live) {
    fit_locate(g, &q);
    auto scan = [&](int cx, int cy, int cz) __attribute__((always_inline)) {
      uint32_t first, end;
      if (!fit_find(tab, g.hash_mask, fit_key(g, cx, cy, cz), &first, &end)) return;
      for (uint32_t s = first; s < end; ++s) {
        const float4 p = pts[s];
        const float dx = p.x - q.qx, dy = p.y - q.qy, dz = p.z - q.qz;
        const float cd = (dx * dx + dy * dy) + dz * dz;
        const int ci = __float_as_int(p.w);
        if (gicp_before(cd, ci, bd, bi)) { bd = cd; bi = ci; }
      }
    };
    fit_walk_box(q, g, scan);
    for (int r = 1;; ++r) {
      if (gicp_settled(bd, fit_lower_bound2(q, g, r), cap2)) break;
      if (r >= r_limit) return false;
      fit_walk_shell(q, g, r + 1, scan);
    }
  }
  const bool keep = live && bi != INT_MAX && bd <= cap2 && tfound[bi] >= GICP_MIN_NEIGHBOURS;
  pair[i] = keep ? bi : -1;
  pd2[i] = keep ? bd : INFINITY;
  if (keep) atomicAdd(&work[W_PAIRS], 1);
  return true;
}

__global__ void __launch_bounds__(GICP_THREADS)
k_gicp_pair(const double* __restrict__ sgauss, int n, GicpMove P, FitGeom g, const float4* __restrict__ pts,
            const uint4* __restrict__ tab, const int32_t* __restrict__ tfound, float cap2, int32_t* __restrict__ pair,
            float* __restrict__ pd2, int* __restrict__ work) {
  const int i = (int)(blockIdx.x * GICP_THREADS + threadIdx.x);
  if (i >= n) return;
  if (gicp_pair_point(i, sgauss, P, g, pts, tab, tfound, cap2, 1, pair, pd2, work)) return;
  work[W_QUEUE + atomicAdd(&work[W_QUEUED], 1)] = i;
}

__global__ void __launch_bounds__(GICP_THREADS)
k_gicp_pair_tail(const double* __restrict__ sgauss, GicpMove P, FitGeom g, const float4* __restrict__ pts,
                 const uint4* __restrict__ tab, const int32_t* __restrict__ tfound, float cap2, int32_t* __restrict__ pair,
                 float* __restrict__ pd2, int* __restrict__ work) {
  const int total = work[W_QUEUED];
  for (int w = (int)(blockIdx.x * GICP_THREADS + threadIdx.x); w < total; w += (int)(gridDim.x * GICP_THREADS))
    gicp_pair_point(work[W_QUEUE + w], sgauss, P, g, pts, tab, tfound, cap2, fit_rmax(g), pair, pd2, work);
}

// One source point per lane: its frozen pair through d2d_pair with the weight -1/2, and the block's row of EV_WORDS sums
// (nvtl_sum = score; word 31 = 0).
template <bool HESSIAN>
__global__ void __launch_bounds__(GICP_THREADS)
k_gicp_eval(const double* __restrict__ sgauss, const int32_t* __restrict__ pair, int n, const double* __restrict__ tgauss,
            D2dPose P, double* __restrict__ rows) {
  __shared__ double s_part[GICP_WAVES][EV_WORDS];
  const int i = (int)(blockIdx.x * GICP_THREADS + threadIdx.x);
  D2dAcc<HESSIAN> acc;
  d2d_acc_clear(acc);
  const int j = i < n ? pair[i] : -1;
  if (j >= 0) {
    const double* G = sgauss + (size_t)i * 9;
    const double mu[3] = {G[0], G[1], G[2]};
    Sym3 S;
    S.xx = G[3]; S.xy = G[4]; S.xz = G[5]; S.yy = G[6]; S.yz = G[7]; S.zz = G[8];
    double m[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = ((P.R[3 * a] * mu[0] + P.R[3 * a + 1] * mu[1]) + P.R[3 * a + 2] * mu[2]) + P.t[a];
    Sym3 A, Z[3];
    double jc[3][3];
    d2d_source_terms(P, mu, S, A, jc, Z);
    d2d_pair<HESSIAN>(acc, tgauss + (size_t)j * 9, m, A, jc, Z, D2dHalfWeight{});
    if (acc.npairs > 0) d2d_second_order(acc, P, mu, S);
  }
  double words[EV_WORDS];
  d2d_words(acc, acc.score, words);
  eval_block_row<GICP_WAVES, HESSIAN>(words, s_part, rows);
}

unsigned blocks_of(size_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

bool gicp_params_valid(const ndt_gicp_params* p) {
  return p && p->k_neighbours >= GICP_MIN_NEIGHBOURS && p->k_neighbours <= 32 && p->max_neighbour_distance > 0.0 &&
         p->covariance_epsilon > 0.0 && p->covariance_epsilon <= 1.0 && p->max_correspondence_distance > 0.0 &&
         std::isfinite(p->transformation_epsilon) && p->transformation_epsilon >= 0.0 && p->max_iterations >= 1 &&
         p->max_inner_iterations >= 1;   // (a NaN fails its comparison)
}

float squared_cap(double cap) { return (float)(cap * cap); }

int gicp_work(ndt_handle* h, size_t n) {
  HIP_TRY(h, h->gicp.work.ensure(n + W_QUEUE));
  HIP_TRY(h, h->gicp.work_h.ensure(W_QUEUE));
  HIP_TRY(h, hipMemsetAsync(h->gicp.work.p, 0, W_QUEUE * sizeof(int), h->stream));
  return NDT_OK;
}

int gicp_work_fetch(ndt_handle* h) {
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(h->gicp.work_h.h, h->gicp.work.p, W_QUEUE * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NDT_OK;
}

// neighbour lists and covariances of the cloud x / y / z (n points) indexed by `f`, under the handle's GICP parameters; awaited
int gicp_derive(ndt_handle* h, GicpCloud& c, const FitIndex& f, const float* x, const float* y, const float* z, size_t n) {
  const ndt_gicp_params& prm = h->gicp.prm;
  c.valid = false;
  if (n > (size_t)std::numeric_limits<int>::max() / 64) return fail(h, NDT_ERR_INVALID_ARG, "GICP: too many points");
  const int k = prm.k_neighbours;
  HIP_TRY(h, c.nbr.ensure(n * (size_t)k));
  HIP_TRY(h, c.nfound.ensure(n));
  HIP_TRY(h, c.mean.ensure(3 * n));
  HIP_TRY(h, c.raw.ensure(6 * n));
  HIP_TRY(h, c.gauss.ensure(9 * n));
  if (int rc = gicp_work(h, n)) return rc;
  hipStream_t s = h->stream;
  const float4* pts = reinterpret_cast<const float4*>(f.pts.p);
  const uint4* tab = reinterpret_cast<const uint4*>(f.tab.p);
  const float cap2 = squared_cap(prm.max_neighbour_distance);
  const dim3 grid(blocks_of(n, KNN_THREADS)), tail(std::min<unsigned>(GICP_TAIL_BLOCKS, blocks_of(n, KNN_THREADS))), block(KNN_THREADS);
  int* work = h->gicp.work.p;
#define NDT_GICP_KNN(KMAX)                                                                                                      \
  {                                                                                                                             \
    hipLaunchKernelGGL(k_gicp_knn<KMAX>, grid, block, 0, s, x, y, z, (int)n, f.g, pts, tab, k, cap2, c.nbr.p, c.nfound.p, work); \
    hipLaunchKernelGGL(k_gicp_knn_tail<KMAX>, tail, block, 0, s, x, y, z, f.g, pts, tab, k, cap2, c.nbr.p, c.nfound.p, work);    \
  }
  if (k <= 8) NDT_GICP_KNN(8) else if (k <= 16) NDT_GICP_KNN(16) else if (k <= 24) NDT_GICP_KNN(24) else NDT_GICP_KNN(32)
#undef NDT_GICP_KNN
  hipLaunchKernelGGL(k_gicp_cov, dim3(blocks_of(n, GICP_THREADS)), dim3(GICP_THREADS), 0, s, x, y, z, (int)n, k, c.nbr.p, c.nfound.p,
                     prm.covariance_epsilon, c.mean.p, c.raw.p, c.gauss.p, work);
  if (int rc = gicp_work_fetch(h)) return rc;
  c.n = n;
  c.k = k;
  c.n_without = h->gicp.work_h.h[W_WITHOUT];
  c.valid = true;
  return NDT_OK;
}

}  // namespace

// (declared in ndt_engine.h: voxelised GICP shares them)
// what every GICP call checks first: one rank, and the streams ordered behind whatever is in flight
int gicp_settle(ndt_handle* h) {
  if (int rc = settle(h)) return rc;
  if (h->red.mode() != NDT_REDUCE_NONE) return fail(h, NDT_ERR_UNSUPPORTED, "GICP: multi-rank evaluation is not supported");
  return NDT_OK;
}

int gicp_target_state(ndt_handle* h) {
  if (h->tgt.is_union())
    return fail(h, NDT_ERR_UNSUPPORTED, "GICP: a multi-grid target keeps no points (set a single target)");
  if (h->tgt.have_grid() && !h->tgt.has_cloud())
    return fail(h, NDT_ERR_UNSUPPORTED,
                "GICP: the target came through ndt_set_target_device* and was consumed there (nothing is retained)");
  if (!h->tgt.have_grid()) return fail(h, NDT_ERR_NO_TARGET, "no target (setInputTarget first)");
  return NDT_OK;
}

int gicp_source_state(ndt_handle* h) {
  if (h->n_src == 0 || !h->vx) return fail(h, NDT_ERR_NO_SOURCE, "no source cloud (setInputSource first)");
  return NDT_OK;
}

// the target's lists and covariances, fresh (the index is the fitness index)
int gicp_target_ready(ndt_handle* h) {
  if (int rc = gicp_target_state(h)) return rc;
  if (int rc = fit_build(h)) return rc;
  GicpCloud& c = h->gicp.tgt;
  if (c.valid && c.gen == h->tgt.gen()) return NDT_OK;
  if (int rc = gicp_derive(h, c, h->fit, h->tx.p, h->ty.p, h->tz.p, h->tgt.cloud_n())) return rc;
  c.gen = h->tgt.gen();
  return NDT_OK;
}

int gicp_source_ready(ndt_handle* h) {
  if (int rc = gicp_source_state(h)) return rc;
  GicpBufs& b = h->gicp;
  if (b.src.valid) return NDT_OK;
  if (!b.sidx.valid) {
    const int rc = fit_build_cloud(h, b.sidx, h->vx, h->vy, h->vz, h->n_src, "GICP: the source");
    if (rc == NDT_ERR_NO_TARGET) return fail(h, NDT_ERR_NO_SOURCE, "GICP: the source has no finite point");
    if (rc) return rc;
  }
  return gicp_derive(h, b.src, b.sidx, h->vx, h->vy, h->vz, h->n_src);
}

namespace {

int gicp_cloud_ready(ndt_handle* h, int which) {
  if (int rc = gicp_settle(h)) return rc;
  return which == NDT_GICP_TARGET ? gicp_target_ready(h) : gicp_source_ready(h);
}

// the pairs at pose6, frozen; both clouds are ready
int gicp_pair(ndt_handle* h, const double pose6[6]) {
  GicpBufs& b = h->gicp;
  b.drop_pairs();
  const size_t n = b.src.n;
  HIP_TRY(h, b.pair.ensure(n));
  HIP_TRY(h, b.pd2.ensure(n));
  if (int rc = gicp_work(h, n)) return rc;
  D2dPose full;
  fill_d2d_pose(pose6, &full);
  GicpMove P;
  std::memcpy(P.R, full.R, sizeof(P.R));
  std::memcpy(P.t, full.t, sizeof(P.t));
  const FitIndex& f = h->fit;
  const float4* pts = reinterpret_cast<const float4*>(f.pts.p);
  const uint4* tab = reinterpret_cast<const uint4*>(f.tab.p);
  const float cap2 = squared_cap(b.prm.max_correspondence_distance);
  const unsigned nb = blocks_of(n, GICP_THREADS);
  hipLaunchKernelGGL(k_gicp_pair, dim3(nb), dim3(GICP_THREADS), 0, h->stream, b.src.gauss.p, (int)n, P, f.g, pts, tab, b.tgt.nfound.p, cap2,
                     b.pair.p, b.pd2.p, b.work.p);
  hipLaunchKernelGGL(k_gicp_pair_tail, dim3(std::min<unsigned>(GICP_TAIL_BLOCKS, nb)), dim3(GICP_THREADS), 0, h->stream, b.src.gauss.p, P, f.g,
                     pts, tab, b.tgt.nfound.p, cap2, b.pair.p, b.pd2.p, b.work.p);
  if (int rc = gicp_work_fetch(h)) return rc;
  b.n_pairs = b.work_h.h[W_PAIRS];
  b.pairs_gen = h->tgt.gen();
  b.pairs_valid = true;
  return NDT_OK;
}

// target, source, then pairs that still describe both
int gicp_eval_ready(ndt_handle* h) {
  if (int rc = gicp_settle(h)) return rc;
  if (int rc = gicp_target_state(h)) return rc;
  if (int rc = gicp_source_state(h)) return rc;
  const GicpBufs& b = h->gicp;
  if (!b.pairs_valid || !b.src.valid || !b.tgt.valid || b.pairs_gen != h->tgt.gen() || b.tgt.gen != h->tgt.gen())
    return fail(h, NDT_ERR_NO_SOURCE, "GICP: no frozen pairs (ndt_gicp_pair first)");
  return NDT_OK;
}

// K poses -> K x EV_WORDS raw sums in `out`; gicp_eval_ready has passed
int gicp_eval_raw(ndt_handle* h, const double* poses6, int K, bool need_h, double* out) {
  GicpBufs& b = h->gicp;
  const int n = (int)b.src.n, nb = (int)blocks_of(b.src.n, GICP_THREADS);
  const dim3 grid((unsigned)nb), block(GICP_THREADS);
  return lane_eval_rows(h, "GICP", nb, K, [&](int k, double* rows) {
    D2dPose P;
    fill_d2d_pose(poses6 + 6 * (size_t)k, &P);
    if (need_h) hipLaunchKernelGGL(k_gicp_eval<true>, grid, block, 0, h->stream, b.src.gauss.p, b.pair.p, n, b.tgt.gauss.p, P, rows);
    else hipLaunchKernelGGL(k_gicp_eval<false>, grid, block, 0, h->stream, b.src.gauss.p, b.pair.p, n, b.tgt.gauss.p, P, rows);
  }, out);
}

template <typename T>
int gicp_download(ndt_handle* h, T* dst, const T* src, size_t count) {
  if (!dst || count == 0) return NDT_OK;
  HIP_TRY(h, hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  return NDT_OK;
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

void ndt_gicp_default_params(ndt_gicp_params* p) {
  if (p) *p = ndt_gicp_params{20, INFINITY, 1e-3, 5.0, 1e-4, 64, 20};
}

int ndt_gicp_set_params(ndt_handle* h, const ndt_gicp_params* p) {
  if (!h || !gicp_params_valid(p)) return NDT_ERR_INVALID_ARG;
  GicpBufs& b = h->gicp;
  const ndt_gicp_params& o = b.prm;
  if (p->k_neighbours != o.k_neighbours || p->max_neighbour_distance != o.max_neighbour_distance ||
      p->covariance_epsilon != o.covariance_epsilon) {
    b.src.valid = b.tgt.valid = false;
    h->vgicp.valid = false;   // (the voxel table is made of the target's covariances)
    b.drop_pairs();
  }
  if (p->max_correspondence_distance != o.max_correspondence_distance) b.drop_pairs();
  b.prm = *p;
  return NDT_OK;
}

int ndt_gicp_get_params(const ndt_handle* h, ndt_gicp_params* p) {
  if (!h || !p) return NDT_ERR_INVALID_ARG;
  *p = h->gicp.prm;
  return NDT_OK;
}

int64_t ndt_gicp_export_neighbours(ndt_handle* h, int which, int32_t* idx, int32_t* n_found, size_t cap) {
  if (!h || (which != NDT_GICP_SOURCE && which != NDT_GICP_TARGET)) return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = gicp_cloud_ready(h, which)) return rc;
  const GicpCloud& c = which == NDT_GICP_TARGET ? h->gicp.tgt : h->gicp.src;
  if (c.n > cap) return over_capacity(h, c.n);
  if (int rc = gicp_download(h, idx, c.nbr.p, c.n * (size_t)c.k)) return rc;
  if (int rc = gicp_download(h, n_found, c.nfound.p, c.n)) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return (int64_t)c.n;
}

int64_t ndt_gicp_export_covariances(ndt_handle* h, int which, double* mean3, double* raw_cov6, double* cov6, size_t cap) {
  if (!h || (which != NDT_GICP_SOURCE && which != NDT_GICP_TARGET)) return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = gicp_cloud_ready(h, which)) return rc;
  const GicpCloud& c = which == NDT_GICP_TARGET ? h->gicp.tgt : h->gicp.src;
  if (c.n > cap) return over_capacity(h, c.n);
  std::vector<double> g(cov6 ? 9 * c.n : 0);
  if (int rc = gicp_download(h, mean3, c.mean.p, 3 * c.n)) return rc;
  if (int rc = gicp_download(h, raw_cov6, c.raw.p, 6 * c.n)) return rc;
  if (int rc = gicp_download(h, cov6 ? g.data() : nullptr, c.gauss.p, 9 * c.n)) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (cov6)
    for (size_t i = 0; i < c.n; ++i) std::memcpy(cov6 + 6 * i, &g[9 * i + 3], 6 * sizeof(double));
  return (int64_t)c.n;
}

int ndt_gicp_pair(ndt_handle* h, const double pose6[6], int64_t* n_pairs) {
  if (!h || !pose6 || !all_finite(pose6, 6)) return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = gicp_settle(h)) return rc;
  if (int rc = gicp_target_ready(h)) return rc;
  if (int rc = gicp_source_ready(h)) return rc;
  if (int rc = gicp_pair(h, pose6)) return rc;
  if (n_pairs) *n_pairs = h->gicp.n_pairs;
  return NDT_OK;
}

int64_t ndt_gicp_export_pairs(ndt_handle* h, int32_t* target_index, float* d2, size_t cap) {
  if (!h) return NDT_ERR_INVALID_ARG;
  const GicpBufs& b = h->gicp;
  if (!b.pairs_valid || !b.src.valid || b.pairs_gen != h->tgt.gen()) return 0;
  if (int rc = bind_device(h)) return rc;
  const size_t n = b.src.n;
  if (n > cap) return over_capacity(h, n);
  if (int rc = gicp_download(h, target_index, b.pair.p, n)) return rc;
  if (int rc = gicp_download(h, d2, b.pd2.p, n)) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return (int64_t)n;
}

int ndt_eval_derivatives_gicp(ndt_handle* h, const double* poses6, int K, int compute_hessian, double* out) {
  if (!h || !poses6 || !out || K <= 0) return NDT_ERR_INVALID_ARG;
  for (int k = 0; k < K; ++k)
    if (!all_finite(poses6 + 6 * (size_t)k, 6)) return NDT_ERR_INVALID_ARG;
  if (int rc = bind_device(h)) return rc;
  if (int rc = gicp_eval_ready(h)) return rc;
  if (int rc = gicp_eval_raw(h, poses6, K, compute_hessian != 0, out)) return rc;
  for (int k = 0; k < K; ++k) finish_words(h, poses6 + 6 * (size_t)k, compute_hessian != 0, out + (size_t)k * EV_WORDS);
  return NDT_OK;
}

int ndt_align_gicp(ndt_handle* h, const float guess[16], ndt_result* out, ndt_gicp_info* info) {
  if (!h || !guess || !out) return NDT_ERR_INVALID_ARG;
  const auto t0 = std::chrono::steady_clock::now();
  const auto give_guess = [&]() {   // what every failure leaves: the guess, not converged
    std::memset(out, 0, sizeof(*out));
    std::memcpy(out->final_transformation, guess, sizeof(float) * 16);
  };
  give_guess();
  if (info) std::memset(info, 0, sizeof(*info));
  if (int rc = bind_device(h)) return rc;
  h->keepwarm.touch();
  if (int rc = gicp_settle(h)) return rc;
  if (int rc = gicp_target_ready(h)) return rc;
  if (int rc = gicp_source_ready(h)) return rc;
  GicpBufs& b = h->gicp;
  ndt_params prm = h->prm;
  prm.trans_epsilon = b.prm.transformation_epsilon;
  prm.max_iterations = b.prm.max_inner_iterations;
  float T[16];
  std::memcpy(T, guess, sizeof(T));
  double p[6];
  matrix_to_pose(T, p);
  if (!all_finite(p, 6)) return fail(h, NDT_ERR_INVALID_ARG, "GICP: the guess is not a finite pose");
  ndt_result r;
  int outer = 0, inner = 0, evals = 0, reused = 0;
  bool converged = false;
  while (outer < b.prm.max_iterations && !converged) {
    if (int rc = gicp_pair(h, p)) { give_guess(); return rc; }
    if (b.n_pairs == 0) { give_guess(); return fail(h, NDT_ERR_NO_SOURCE, "GICP: no pair within max_correspondence_distance"); }
    const int rc = lane_align(h, (int64_t)h->n_src, T,
                              [h](const double* q, bool need_h, double* words) { return gicp_eval_raw(h, q, 1, need_h, words); }, &r, &prm);
    if (rc) { give_guess(); return rc; }
    ++outer;
    inner += r.iterations;
    evals += r.n_evaluations;
    reused += r.n_evaluations_reused;
    double len = 0.0;
    for (int c = 0; c < 6; ++c) len += (r.final_pose[c] - p[c]) * (r.final_pose[c] - p[c]);
    converged = std::sqrt(len) < b.prm.transformation_epsilon;
    std::memcpy(p, r.final_pose, sizeof(p));
    std::memcpy(T, r.final_transformation, sizeof(T));
  }
  *out = r;
  out->converged = converged ? 1 : 0;
  out->iterations = outer;
  out->n_evaluations = evals;
  out->n_evaluations_reused = reused;
  out->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (info) {
    info->outer_iterations = outer;
    info->inner_iterations = inner;
    info->n_evaluations = evals;
    info->n_pairs = b.n_pairs;
    info->n_source_without_covariance = b.src.n_without;
    info->n_target_without_covariance = b.tgt.n_without;
  }
  return NDT_OK;
}

}  // extern "C"
