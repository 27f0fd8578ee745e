// ndt_fitness.hip -- getFitnessScore: the mean squared distance from every transformed source point to its nearest RAW
// target point (see include/ndt_hip.h and DESIGN.md section 7a).  The voxel grid cannot answer it (leaves keep centroids
// of voxels with >= min_points_per_voxel points), so the engine keeps a second, point-level index over its own copy of
// the target (tx / ty / tz), built lazily by the first fitness call after the target changed:
//   - cells of edge c (the grid resolution, grown until the bounding box has < 2^30 cells) on the bounding box of the
//     finite target points, keys relative to its minimum;
//   - the finite points stably sorted by cell (the engine's radix sort over the index's own buffers), as float4;
//   - an open-addressing hash table of the occupied cells: {key, first point, end point}.  Memory is O(points), never
//     O(bounding volume).
// Query: one lane per (source point, pose).  Pass 1 scans the 27 cells around the point and stops when the best d^2
// is at most the squared lower bound on the distance to every cell not yet scanned (fit_lower_bound2); the rest is
// compacted and finished by pass 2, which scans Chebyshev shells r = 2, 3, ... restricted to the bounding box.  Then a
// fixed-order f64 reduction per pose (per-block partial sums in a slab, added on the host in block order): no float
// atomics, bit-reproducible.
#include "ndt_engine.h"
#include "ndt_fit_device.h"

namespace ndt {
namespace engine {
namespace {

constexpr int FIT_THREADS = 256;
constexpr int FIT_BOUNDS_BLOCKS = 256;
constexpr int FIT_REDUCE_CHUNK = 2048;       // points per reduction block (8 per lane)
constexpr int FIT_SHELL_BLOCKS = 1024;       // pass 2: grid-stride over the compacted entries

__global__ void __launch_bounds__(FIT_THREADS) k_fit_bounds(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, int n, float* __restrict__ bslab,
                                                            int* __restrict__ cslab) {
  __shared__ float smin[3][FIT_THREADS], smax[3][FIT_THREADS];
  __shared__ int scnt[FIT_THREADS];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int cnt = 0;
  for (int i = blockIdx.x * FIT_THREADS + threadIdx.x; i < n; i += gridDim.x * FIT_THREADS) {
    const float px = x[i], py = y[i], pz = z[i];
    if (!finite3(px, py, pz)) continue;
    lo[0] = fminf(lo[0], px); lo[1] = fminf(lo[1], py); lo[2] = fminf(lo[2], pz);
    hi[0] = fmaxf(hi[0], px); hi[1] = fmaxf(hi[1], py); hi[2] = fmaxf(hi[2], pz);
    ++cnt;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) { smin[a][threadIdx.x] = lo[a]; smax[a][threadIdx.x] = hi[a]; }
  scnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int s = FIT_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        smin[a][threadIdx.x] = fminf(smin[a][threadIdx.x], smin[a][threadIdx.x + s]);
        smax[a][threadIdx.x] = fmaxf(smax[a][threadIdx.x], smax[a][threadIdx.x + s]);
      }
      scnt[threadIdx.x] += scnt[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { bslab[6 * blockIdx.x + a] = smin[a][0]; bslab[6 * blockIdx.x + 3 + a] = smax[a][0]; }
    cslab[blockIdx.x] = scnt[0];
  }
}

__global__ void __launch_bounds__(FIT_THREADS) k_fit_keys(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ z, int n, FitGeom g,
                                                          uint32_t* __restrict__ keys) {
  const int i = blockIdx.x * FIT_THREADS + threadIdx.x;
  if (i >= n) return;
  const float px = x[i], py = y[i], pz = z[i];
  uint32_t key = g.ncells;   // non-finite: sorts behind every finite point
  if (finite3(px, py, pz)) {
    const int cx = min(max(fit_cell((px - g.lo[0]) * g.inv_c, g.dims[0]), 0), g.dims[0] - 1);
    const int cy = min(max(fit_cell((py - g.lo[1]) * g.inv_c, g.dims[1]), 0), g.dims[1] - 1);
    const int cz = min(max(fit_cell((pz - g.lo[2]) * g.inv_c, g.dims[2]), 0), g.dims[2] - 1);
    key = fit_key(g, cx, cy, cz);
  }
  keys[i] = key;
}

// the finite points in cell order as float4, w = the point's input index (its bits); the first point of every cell claims
// a hash slot and records itself
__global__ void __launch_bounds__(FIT_THREADS) k_fit_gather(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, const uint32_t* __restrict__ sorted_keys,
                                                            const uint32_t* __restrict__ sorted_vals, int nf, uint32_t mask,
                                                            float4* __restrict__ pts, uint32_t* __restrict__ tab) {
  const int i = blockIdx.x * FIT_THREADS + threadIdx.x;
  if (i >= nf) return;
  const uint32_t key = sorted_keys[i], idx = sorted_vals[i];
  pts[i] = make_float4(x[idx], y[idx], z[idx], __int_as_float((int)idx));
  if (i > 0 && sorted_keys[i - 1] == key) return;
  uint32_t slot = fit_hash(key, mask);
  for (;;) {   // (the table has at least twice as many slots as there are cells)
    if (atomicCAS(&tab[4 * (size_t)slot], FIT_EMPTY, key) == FIT_EMPTY) { tab[4 * (size_t)slot + 1] = (uint32_t)i; return; }
    slot = (slot + 1) & mask;
  }
}

// the last point of every cell writes the cell's end (the slots were all claimed by the previous launch)
__global__ void __launch_bounds__(FIT_THREADS) k_fit_ends(const uint32_t* __restrict__ sorted_keys, int nf, uint32_t mask,
                                                          uint32_t* __restrict__ tab) {
  const int i = blockIdx.x * FIT_THREADS + threadIdx.x;
  if (i >= nf) return;
  const uint32_t key = sorted_keys[i];
  if (i + 1 < nf && sorted_keys[i + 1] == key) return;
  uint32_t slot = fit_hash(key, mask);
  while (tab[4 * (size_t)slot] != key) slot = (slot + 1) & mask;
  tab[4 * (size_t)slot + 2] = (uint32_t)(i + 1);
}

__device__ __forceinline__ bool fit_transform(const float* __restrict__ P, float x, float y, float z, const FitGeom& g,
                                              FitQuery* q) {
  // exactly k_transform (ndt_derivs.hip): same operations, same order, -ffp-contract=off
  q->qx = P[0] * x + (P[1] * y + (P[2] * z + P[9]));
  q->qy = P[3] * x + (P[4] * y + (P[5] * z + P[10]));
  q->qz = P[6] * x + (P[7] * y + (P[8] * z + P[11]));
  if (!finite3(q->qx, q->qy, q->qz)) return false;
  fit_locate(g, q);
  return true;
}

__device__ __forceinline__ void fit_scan_cell(const float4* __restrict__ pts, const uint4* __restrict__ tab,
                                              const FitGeom& g, int cx, int cy, int cz, const FitQuery& q, float* best) {
  uint32_t first, end;
  if (!fit_find(tab, g.hash_mask, fit_key(g, cx, cy, cz), &first, &end)) return;
  float b = *best;
  for (uint32_t j = first; j < end; ++j) {
    const float4 p = pts[j];
    const float dx = p.x - q.qx, dy = p.y - q.qy, dz = p.z - q.qz;
    const float d2 = dx * dx + dy * dy + dz * dz;
    b = fminf(b, d2);
  }
  *best = b;
}

// verdict of a point after its box of radius r: 1 = done (d2 final), 0 = search on
__device__ __forceinline__ int fit_settle(float best, float lb2, double max_range, float* d2) {
  if (best <= lb2) { *d2 = (double)best > max_range ? INFINITY : best; return 1; }
  if ((double)lb2 > max_range) { *d2 = INFINITY; return 1; }   // nothing within sqrt(max_range) is left: outlier
  return 0;
}

// pass 1: one lane per (point i, pose blockIdx.y); the 27 cells around the point
__global__ void __launch_bounds__(FIT_THREADS) k_fit_query(const float* __restrict__ sx, const float* __restrict__ sy,
                                                           const float* __restrict__ sz, int n,
                                                           const float* __restrict__ poses, FitGeom g,
                                                           const float4* __restrict__ pts, const uint4* __restrict__ tab,
                                                           double max_range, float* __restrict__ dist,
                                                           int* __restrict__ work) {
  const int i = blockIdx.x * FIT_THREADS + threadIdx.x;
  if (i >= n) return;
  const size_t e = (size_t)blockIdx.y * n + i;
  FitQuery q;
  if (!fit_transform(poses + 12 * blockIdx.y, sx[i], sy[i], sz[i], g, &q)) { dist[e] = NAN; return; }
  float best = INFINITY;
  fit_walk_box(q, g, [&](int cx, int cy, int cz) { fit_scan_cell(pts, tab, g, cx, cy, cz, q, &best); });
  float d2;
  if (fit_settle(best, fit_lower_bound2(q, g, 1), max_range, &d2)) { dist[e] = d2; return; }
  dist[e] = best;                      // (the best so far; pass 2 goes on from it)
  work[1 + atomicAdd(&work[0], 1)] = (int)e;
}

// pass 2: the compacted unresolved entries, Chebyshev shells r = 2, 3, ... clipped to the grid
__global__ void __launch_bounds__(FIT_THREADS) k_fit_shells(const float* __restrict__ sx, const float* __restrict__ sy,
                                                            const float* __restrict__ sz, int n,
                                                            const float* __restrict__ poses, FitGeom g,
                                                            const float4* __restrict__ pts, const uint4* __restrict__ tab,
                                                            double max_range, float* __restrict__ dist,
                                                            const int* __restrict__ work) {
  const int total = work[0];
  for (int w = blockIdx.x * FIT_THREADS + threadIdx.x; w < total; w += gridDim.x * FIT_THREADS) {
    const int e = work[1 + w];
    const int k = e / n, i = e - k * n;
    FitQuery q;
    fit_transform(poses + 12 * k, sx[i], sy[i], sz[i], g, &q);   // (finite: pass 1 queued it)
    float best = dist[e], d2 = best;
    const int rmax = fit_rmax(g);
    for (int r = 2; r <= rmax; ++r) {
      fit_walk_shell(q, g, r, [&](int cx, int cy, int cz) { fit_scan_cell(pts, tab, g, cx, cy, cz, q, &best); });
      if (fit_settle(best, fit_lower_bound2(q, g, r), max_range, &d2)) break;
    }
    dist[e] = d2;
  }
}

// fixed-order partial sums: block (b, pose y) adds points [b * CHUNK, (b + 1) * CHUNK) of pose y -- lane t the points
// t, t + 256, ... in order, then a fixed LDS tree -- into slab row (y, b) = {sum d^2, inliers, finite points}
__global__ void __launch_bounds__(FIT_THREADS) k_fit_reduce(const float* __restrict__ dist, int n,
                                                            double* __restrict__ slab) {
  __shared__ double ssum[FIT_THREADS], sin_[FIT_THREADS], spts[FIT_THREADS];
  const float* d = dist + (size_t)blockIdx.y * n;
  const int begin = blockIdx.x * FIT_REDUCE_CHUNK, end = min(begin + FIT_REDUCE_CHUNK, n);
  double s = 0.0, ni = 0.0, np = 0.0;
  for (int i = begin + (int)threadIdx.x; i < end; i += FIT_THREADS) {
    const float v = d[i];
    if (isnan(v)) continue;
    np += 1.0;
    if (isinf(v)) continue;
    s += (double)v;
    ni += 1.0;
  }
  ssum[threadIdx.x] = s; sin_[threadIdx.x] = ni; spts[threadIdx.x] = np;
  __syncthreads();
  for (int st = FIT_THREADS / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      ssum[threadIdx.x] += ssum[threadIdx.x + st];
      sin_[threadIdx.x] += sin_[threadIdx.x + st];
      spts[threadIdx.x] += spts[threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* row = slab + 3 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
    row[0] = ssum[0]; row[1] = sin_[0]; row[2] = spts[0];
  }
}

unsigned grid1(size_t n) { return (unsigned)((n + FIT_THREADS - 1) / FIT_THREADS); }

}  // namespace

// (Re)builds the index `f` over the SoA cloud x / y / z (device memory, n points) on the engine's stream; `what` heads
// the error texts.  The caller tags the index (gen) when that is how it is kept fresh.
int fit_build_cloud(ndt_handle* h, FitIndex& f, const float* x, const float* y, const float* z, size_t n, const char* what) {
  f.valid = false;
  hipStream_t s = h->stream;
  // bounds of the finite points: per-block rows, finished on the host (one wait: the geometry sizes everything else)
  const int nb = (int)std::min<size_t>(FIT_BOUNDS_BLOCKS, grid1(n));
  HIP_TRY(h, f.bslab.ensure(6 * (size_t)nb));
  HIP_TRY(h, f.cslab.ensure(nb));
  HIP_TRY(h, f.bslab_h.ensure(6 * FIT_BOUNDS_BLOCKS));
  HIP_TRY(h, f.cslab_h.ensure(FIT_BOUNDS_BLOCKS));
  hipLaunchKernelGGL(k_fit_bounds, dim3((unsigned)nb), dim3(FIT_THREADS), 0, s, x, y, z, (int)n, f.bslab.p, f.cslab.p);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(f.bslab_h.h, f.bslab.p, 6 * (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(f.cslab_h.h, f.cslab.p, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int64_t nf = 0;
  for (int b = 0; b < nb; ++b) {
    if (f.cslab_h.h[b] <= 0) continue;
    nf += f.cslab_h.h[b];
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], f.bslab_h.h[6 * b + a]);
      hi[a] = std::max(hi[a], f.bslab_h.h[6 * b + 3 + a]);
    }
  }
  if (nf == 0) return fail(h, NDT_ERR_NO_TARGET, std::string(what) + " has no finite point");
  // cell edge: the grid resolution (a cell then holds about what a voxel holds), grown until the bounding box has
  // fewer than 2^30 cells (the keys are 32-bit and the radix sort sorts 32-bit keys; the table never sees empty cells)
  FitGeom g{};
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(hi[a] - lo[a])) return fail(h, NDT_ERR_UNSUPPORTED, std::string(what) + "'s extent overflows f32");
  float c = h->prm.resolution;
  for (;;) {
    const float inv_c = 1.0f / c;
    double d[3], cells = 1.0;
    for (int a = 0; a < 3; ++a) {
      const float u = (hi[a] - lo[a]) * inv_c;    // the device's f32 arithmetic: the last cell holds hi
      d[a] = (double)std::floor(u) + 1.0;
      cells *= d[a];
    }
    if (cells < (double)(1u << 30)) {
      for (int a = 0; a < 3; ++a) g.dims[a] = (int)d[a];
      g.c = c; g.inv_c = inv_c; g.ncells = (uint32_t)cells;
      break;
    }
    c *= 1.25f;
  }
  for (int a = 0; a < 3; ++a) g.lo[a] = lo[a];
  g.n_finite = (int)nf;
  uint32_t slots = 1024;
  while (slots < 2 * (uint64_t)nf) slots <<= 1;
  g.hash_mask = slots - 1;
  // stable sort of (cell key, point) -- non-finite points carry the key ncells and sort behind the finite ones
  HIP_TRY(h, f.sort.ensure(n));
  HIP_TRY(h, f.plan.ensure(1));
  HIP_TRY(h, f.pts.ensure(4 * (size_t)nf));
  HIP_TRY(h, f.tab.ensure(4 * (size_t)slots));
  int passes = 0;
  if (int rc = sort_put_plan(h, f.plan.p, sort_key_bits(g.ncells), 0, &passes)) return rc;   // (the last key is `ncells`)
  hipLaunchKernelGGL(k_fit_keys, dim3(grid1(n)), dim3(FIT_THREADS), 0, s, x, y, z, (int)n, g, f.sort.keys.p);
  SortedPairs sorted;
  HIP_TRY(h, sort_keyed(f.sort, n, f.plan.p, passes, SORT_COUNT_FIRST, s, &sorted));
  const uint32_t *sk = sorted.keys, *sv = sorted.vals;
  HIP_TRY(h, hipMemsetAsync(f.tab.p, 0xff, 4 * (size_t)slots * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_fit_gather, dim3(grid1((size_t)nf)), dim3(FIT_THREADS), 0, s, x, y, z, sk, sv, (int)nf, g.hash_mask,
                     reinterpret_cast<float4*>(f.pts.p), f.tab.p);
  hipLaunchKernelGGL(k_fit_ends, dim3(grid1((size_t)nf)), dim3(FIT_THREADS), 0, s, sk, (int)nf, g.hash_mask, f.tab.p);
  HIP_TRY(h, hipGetLastError());
  f.g = g;
  f.valid = true;
  return NDT_OK;
}

// Lazily (re)builds the index over the engine's copy of the target.  Called with the target settled.
int fit_build(ndt_handle* h) {
  FitIndex& f = h->fit;
  if (f.valid && f.gen == h->tgt.gen()) return NDT_OK;
  if (int rc = fit_build_cloud(h, f, h->tx.p, h->ty.p, h->tz.p, h->tgt.cloud_n(), "fitness: the target")) return rc;
  f.gen = h->tgt.gen();
  return NDT_OK;
}

namespace {

// argument checks that need no device, then the state checks of the C-ABI's table
int fit_ready(ndt_handle* h) {
  int rc = bind_device(h);
  if (rc) return rc;
  rc = settle(h);   // orders the engine's stream behind the target's upload, the pending build and the source upload
  if (rc) return rc;
  if (h->tgt.is_union())
    return fail(h, NDT_ERR_UNSUPPORTED, "fitness: a multi-grid target keeps no points (set a single target)");
  if (h->tgt.have_grid() && !h->tgt.has_cloud())
    return fail(h, NDT_ERR_UNSUPPORTED,
                "fitness: the target came through ndt_set_target_device* and was consumed there (nothing is retained)");
  if (!h->tgt.have_grid()) return fail(h, NDT_ERR_NO_TARGET, "no target (setInputTarget first)");
  if (h->n_src == 0 && h->red.mode() == NDT_REDUCE_NONE)
    return fail(h, NDT_ERR_NO_SOURCE, "no source cloud (setInputSource first)");
  return fit_build(h);
}

void pose12(const float* T, float* P) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) P[3 * i + j] = T[4 * j + i];   // (as ndt_transform_source fills PoseConsts)
    P[9 + i] = T[12 + i];
  }
}

int fit_query(ndt_handle* h, const float* T, int K, double max_range, ndt_fitness* out, float* sq, size_t cap) {
  FitIndex& f = h->fit;
  const size_t n = h->n_src;
  for (int k = 0; k < K; ++k) out[k] = ndt_fitness{std::numeric_limits<double>::max(), 0.0, 0, 0};
  if (n == 0) return NDT_OK;   // (an empty shard of a sharded source)
  if ((size_t)K * n > (size_t)std::numeric_limits<int>::max() - 1)
    return fail(h, NDT_ERR_INVALID_ARG, "fitness: K x source points exceeds 2^31 - 2");
  hipStream_t s = h->stream;
  const int nred = (int)((n + FIT_REDUCE_CHUNK - 1) / FIT_REDUCE_CHUNK);
  HIP_TRY(h, f.dist.ensure((size_t)K * n));
  HIP_TRY(h, f.work.ensure((size_t)K * n + 1));
  HIP_TRY(h, f.poses.ensure(12 * (size_t)K));
  HIP_TRY(h, f.slab.ensure(3 * (size_t)K * nred));
  HIP_TRY(h, f.slab_h.ensure(3 * (size_t)K * nred));
  std::vector<float> P(12 * (size_t)K);
  for (int k = 0; k < K; ++k) pose12(T + 16 * (size_t)k, &P[12 * (size_t)k]);
  HIP_TRY(h, hipMemcpyAsync(f.poses.p, P.data(), P.size() * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemsetAsync(f.work.p, 0, sizeof(int), s));
  const float4* pts = reinterpret_cast<const float4*>(f.pts.p);
  const uint4* tab = reinterpret_cast<const uint4*>(f.tab.p);
  hipLaunchKernelGGL(k_fit_query, dim3(grid1(n), (unsigned)K), dim3(FIT_THREADS), 0, s, h->vx, h->vy, h->vz, (int)n,
                     f.poses.p, f.g, pts, tab, max_range, f.dist.p, f.work.p);
  const unsigned nsh = (unsigned)std::min<size_t>(FIT_SHELL_BLOCKS, grid1((size_t)K * n));
  hipLaunchKernelGGL(k_fit_shells, dim3(nsh), dim3(FIT_THREADS), 0, s, h->vx, h->vy, h->vz, (int)n, f.poses.p, f.g, pts,
                     tab, max_range, f.dist.p, f.work.p);
  hipLaunchKernelGGL(k_fit_reduce, dim3((unsigned)nred, (unsigned)K), dim3(FIT_THREADS), 0, s, f.dist.p, (int)n, f.slab.p);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(f.slab_h.h, f.slab.p, 3 * (size_t)K * nred * sizeof(double), hipMemcpyDeviceToHost, s));
  if (sq) HIP_TRY(h, hipMemcpyAsync(sq, f.dist.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  (void)cap;
  for (int k = 0; k < K; ++k) {   // block order: the same bits for every call
    double sum = 0.0, ni = 0.0, np = 0.0;
    for (int b = 0; b < nred; ++b) {
      const double* row = f.slab_h.h + 3 * ((size_t)k * nred + b);
      sum += row[0]; ni += row[1]; np += row[2];
    }
    out[k].sum_sq_dist = sum;
    out[k].n_inliers = (int64_t)ni;
    out[k].n_points = (int64_t)np;
    out[k].fitness_score = ni > 0 ? sum / ni : std::numeric_limits<double>::max();
  }
  return NDT_OK;
}

bool range_ok(double max_range) { return !std::isnan(max_range) && max_range >= 0.0; }

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

int ndt_fitness_score(ndt_handle* h, const float T[16], double max_range, ndt_fitness* out, float* sq_dists_out,
                      size_t cap) {
  if (!h || !T || !out) return NDT_ERR_INVALID_ARG;
  if (!range_ok(max_range)) return fail(h, NDT_ERR_INVALID_ARG, "fitness: max_range must be >= 0 (a squared distance)");
  if (sq_dists_out && cap < h->n_src) return fail(h, NDT_ERR_INVALID_ARG, "fitness: sq_dists_out holds fewer than n_source");
  int rc = fit_ready(h);
  if (rc) return rc;
  return fit_query(h, T, 1, max_range, out, sq_dists_out, cap);
}

int ndt_fitness_scores(ndt_handle* h, const float* transforms, int K, double max_range, ndt_fitness* out) {
  if (!h || !transforms || !out || K < 1) return NDT_ERR_INVALID_ARG;
  if (K > 65535) return fail(h, NDT_ERR_INVALID_ARG, "fitness: at most 65535 transforms per call");
  if (!range_ok(max_range)) return fail(h, NDT_ERR_INVALID_ARG, "fitness: max_range must be >= 0 (a squared distance)");
  int rc = fit_ready(h);
  if (rc) return rc;
  return fit_query(h, transforms, K, max_range, out, nullptr, 0);
}

}  // extern "C"
