// ndt_sort.hip -- the engine's keyed sort: the stable LSD radix sort of (key, index) pairs in launch-per-phase digit
// passes (count / scan / scatter, tile shape: ndt_sort_device.h), its plan on the host (rule: ndt_sort_plan.h), and what
// its users on a handle share around it -- the scratch (SortScratch, ndt_engine.h), the one sort call (sort_keyed), and
// the run search behind it (group_scratch, find_runs; the kernels k_runs stay with the build in ndt_target.hip).
// Users: the target build's sort-based path, ndt_voxel_downsample*, the voxel map (add / import / levels / export order),
// the fitness index, the source ordering, ndt_debug_sort_pairs.
#include "ndt_engine.h"
#include "ndt_sort_device.h"

namespace ndt {

namespace {

__global__ void __launch_bounds__(SORT_THREADS) k_sort_count(const uint32_t* __restrict__ keys, int n, int pass,
                                                            const BuildGeom* __restrict__ gd, int ntiles,
                                                            int* __restrict__ hist) {
  __shared__ int h[SORT_BINS];
  if (gd->status != BG_OK) return;
  const int shift = gd->shift[pass];
  const uint32_t digit_mask = (1u << gd->width[pass]) - 1u;
  h[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t key[SORT_ROUNDS];
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int i = sort_index(blockIdx.x, wave, r, lane);
    key[r] = keys[i < n ? i : 0];
  }
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r)
    if (sort_index(blockIdx.x, wave, r, lane) < n) atomicAdd(&h[(key[r] >> shift) & digit_mask], 1);
  __syncthreads();
  hist[threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// one block per bin: exclusive scan of that bin's counts over the tiles (in place) + total
__global__ void __launch_bounds__(SORT_THREADS) k_sort_scan(int* __restrict__ hist, int ntiles, int* __restrict__ totals) {
  __shared__ int wsum[SORT_WAVES];
  __shared__ int carry;
  int* row = hist + (size_t)blockIdx.x * ntiles;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int base = 0; base < ntiles; base += SORT_THREADS) {
    const int i = base + threadIdx.x;
    const int v = i < ntiles ? row[i] : 0;
    const int incl = wave_inclusive_scan(v, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (i < ntiles) row[i] = before + incl - v;
    __syncthreads();
    if (threadIdx.x == SORT_THREADS - 1) carry = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// FIRST: the values are the identity permutation and are synthesised instead of read
template <bool FIRST>
__global__ void __launch_bounds__(SORT_THREADS) k_sort_scatter(const uint32_t* __restrict__ keys_in,
                                                              const uint32_t* __restrict__ vals_in, int n, int pass,
                                                              const BuildGeom* __restrict__ gd, int ntiles,
                                                              const int* __restrict__ hist,
                                                              const int* __restrict__ totals,
                                                              uint32_t* __restrict__ keys_out,
                                                              uint32_t* __restrict__ vals_out) {
  __shared__ int cnt[SORT_WAVES][SORT_BINS];
  __shared__ int gbase[SORT_BINS];
  __shared__ int wsum[SORT_WAVES];
  if (gd->status != BG_OK) return;
  const int shift = gd->shift[pass];
  const uint32_t digit_mask = (1u << gd->width[pass]) - 1u;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {  // first output slot of every digit for this tile: bins before it + same bin in earlier tiles
    const int t = totals[threadIdx.x];
    const int incl = wave_inclusive_scan(t, lane);
    if (lane == 63) wsum[wave] = incl;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) cnt[w][threadIdx.x] = 0;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    gbase[threadIdx.x] = before + incl - t + hist[threadIdx.x * ntiles + blockIdx.x];
  }
  uint32_t key[SORT_ROUNDS], val[SORT_ROUNDS];
  int rank[SORT_ROUNDS];
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int i = sort_index(blockIdx.x, wave, r, lane);
    key[r] = i < n ? keys_in[i] : 0u;
    val[r] = FIRST ? (uint32_t)i : (i < n ? vals_in[i] : 0u);
  }
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const bool valid = sort_index(blockIdx.x, wave, r, lane) < n;
    const uint32_t d = (key[r] >> shift) & digit_mask;
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const int before = cnt[wave][d];
    const int lower = __popcll(same & lt_mask);
    rank[r] = before + lower;
    __builtin_amdgcn_wave_barrier();
    if (valid && lower == 0) cnt[wave][d] = before + __popcll(same);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    int run = 0;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) {
      const int t = cnt[w][threadIdx.x];
      cnt[w][threadIdx.x] = run;
      run += t;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    if (sort_index(blockIdx.x, wave, r, lane) >= n) break;
    const uint32_t d = (key[r] >> shift) & digit_mask;
    const int pos = gbase[d] + cnt[wave][d] + rank[r];
    keys_out[pos] = key[r];
    vals_out[pos] = val[r];
  }
}

}  // namespace

int sort_tiles(size_t n) { return (int)((n + SORT_TILE - 1) / SORT_TILE); }

// scratch of the sort: the bin-major tile histograms + the bin totals
size_t sort_temp_bytes(size_t n) { return ((size_t)SORT_BINS * sort_tiles(n) + SORT_BINS) * sizeof(int); }

int sort_passes_for_cells(long long ncells) {   // the sentinel key is `ncells`
  return sort_passes_for_bits(std::min(32, std::max(1, sort_key_bits(ncells))));
}

namespace engine {

hipError_t SortScratch::ensure(size_t n) {
  hipError_t e = keys.ensure(n);
  if (e == hipSuccess) e = vals.ensure(n);
  if (e == hipSuccess) e = keys2.ensure(n);
  if (e == hipSuccess) e = vals2.ensure(n);
  if (e == hipSuccess) e = tmp.ensure(sort_temp_bytes(n));
  return e;
}

int sort_put_plan(ndt_handle* h, BuildGeom* d_plan, int bits, int ncells, int* passes) {
  HIP_TRY(h, h->plan_h.ensure(SORT_PLAN_SLOTS));
  if (h->plan_next == SORT_PLAN_SLOTS) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->plan_next = 0;
  }
  BuildGeom& b = h->plan_h.h[h->plan_next++];
  b = BuildGeom{};
  b.bits = std::min(32, std::max(1, bits));
  b.passes = sort_passes_for_bits(b.bits);
  sort_split_bits(b.bits, b.passes, b.width, b.shift);
  b.g.ncells = ncells;
  b.status = BG_OK;
  *passes = b.passes;
  HIP_TRY(h, hipMemcpyAsync(d_plan, &b, sizeof(BuildGeom), hipMemcpyHostToDevice, h->stream));
  return NDT_OK;
}

hipError_t sort_keyed(SortScratch& sc, size_t n, const BuildGeom* d_plan, int passes, SortFirstDigit first, hipStream_t s,
                      SortedPairs* out) {
  // the passes ping-pong between the scratch's two pairs of arrays: what the last one wrote is the result
  uint32_t *kin = sc.keys.p, *kout = sc.keys2.p, *vin = sc.vals.p, *vout = sc.vals2.p;
  const int ntiles = sort_tiles(n);
  int* hist = reinterpret_cast<int*>(sc.tmp.p);
  int* totals = hist + (size_t)SORT_BINS * ntiles;
  for (int p = 0; p < passes && n != 0; ++p) {
    if (p > 0 || first == SORT_COUNT_FIRST)
      hipLaunchKernelGGL(k_sort_count, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, s, kin, (int)n, p, d_plan, ntiles, hist);
    hipLaunchKernelGGL(k_sort_scan, dim3(SORT_BINS), dim3(SORT_THREADS), 0, s, hist, ntiles, totals);
    if (p == 0)
      hipLaunchKernelGGL(k_sort_scatter<true>, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, s, kin, vin, (int)n, p, d_plan,
                         ntiles, hist, totals, kout, vout);
    else
      hipLaunchKernelGGL(k_sort_scatter<false>, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, s, kin, vin, (int)n, p, d_plan,
                         ntiles, hist, totals, kout, vout);
    std::swap(kin, kout);
    std::swap(vin, vout);
  }
  *out = SortedPairs{kin, vin};
  return n != 0 ? hipGetLastError() : hipSuccess;
}

int group_scratch(ndt_handle* h, size_t n, size_t max_runs) {
  HIP_TRY(h, h->gd.ensure(1));
  HIP_TRY(h, h->gdh.ensure(1));
  if (!h->tickets.p) {
    HIP_TRY(h, h->tickets.ensure(6));
    HIP_TRY(h, hipMemsetAsync(h->tickets.p, 0, h->tickets.cap * sizeof(unsigned int), h->stream));
  }
  HIP_TRY(h, h->nleaf.ensure(4));  // [0] slots, [1] valid, [2] buckets that declined (two-launch build)
  HIP_TRY(h, h->plan_h.ensure(SORT_PLAN_SLOTS));   // (here, not in a caller's sort_put_plan behind its first write)
  HIP_TRY(h, h->sort.ensure(n));
  HIP_TRY(h, h->leaf_start.ensure(max_runs));
  HIP_TRY(h, h->leaf_cnt.ensure(max_runs));
  HIP_TRY(h, h->run_counts.ensure((size_t)runs_blocks(n)));
  HIP_TRY(h, h->run_offsets.ensure((size_t)runs_blocks(n)));
  return NDT_OK;
}

hipError_t find_runs(ndt_handle* h, const uint32_t* keys_sorted, size_t n, int min_pts, bool fused) {
  return launch_find_runs(keys_sorted, n, h->gd.p, h->gdh.d, min_pts, h->nleaf.p, h->run_counts.p, h->run_offsets.p,
                          h->tickets.p + 1, fused ? h->run_tags.p : nullptr, h->run_tags.cap, &h->run_seq, h->leaf_start.p,
                          h->leaf_cnt.p, h->stream);
}

}  // namespace engine
}  // namespace ndt
