// ndt_map_components.hip -- connected components of the voxel map (ndt_map_components*, ndt_map_export_labels*,
// ndt_map_label_points*, ndt_map_remove_components; see ndt_engine.h: VoxelMap): which occupied voxels belong together
// under 6 / 18 / 26 adjacency, as integers per table slot.  A fixed number of launches whatever the components' diameters:
//   init     parent[slot] = slot for an eligible slot (occupied, count >= min_count), CC_NONE for the rest; label = -1
//   link     one lane per eligible slot probes the FORWARD half of its neighbourhood (the 3 / 9 / 13 offsets with the
//            larger key, map_find: read only) and unites the two sets in a lock-free union-find
//   flatten  a launch of its own (it reads what link wrote): parent[slot] = the set's root
//   number   the occupied slots in ascending key order (map_export_order); a root is the first voxel of its component in
//            that order, so its number is the exclusive count of roots before it: the shared compaction (count / scan /
//            position, ONE host wait for C) -- the root's lane also writes its record's root_ijk and neutral words
//   reduce   one pass over the slots: label = the root's label; the record's voxel count, 64-bit point total and ijk box
//            by integer atomics, one per word (equal labels of a wave folded first)
//   move     the crop's move under the survive predicate: a survivor flag per component, a label per slot
//   label_points   one lane per point: the add's transform and voxel, one map_find, one label load
// THE UNION-FIND.  parent[] is one uint32 per slot (MAP_MAX_CAPACITY = 2^30).  The only order is the voxel key: a hook
// puts the root with the LARGER key under a node of the other set with a SMALLER key, by atomicCAS(parent + r, r, other),
// which succeeds only while r is a root.  Hence (I1) along parent pointers keys strictly fall, so there is no cycle and a
// set's root is its smallest key -- the rule's root; (I2) parent[x] leaves the value x once, by that CAS, and never
// returns to it; (I3) every value parent[x] ever held is a node of x's set with a key <= x's.  Path halving stores a
// grandparent, which keeps all three.  A load of parent may therefore be STALE (MI355X: a CU's L1 is not refreshed by
// another CU's stores) and the algorithm stays correct: a stale value is an earlier value, by I3 still a node of the same
// set further up in key order; climbing ends at a node that looked like a root, and only the CAS tells whether it is one
// -- a failed CAS returns the true parent and the loop goes on FROM THAT VALUE.  On top of that the loads and the halving
// stores of link are relaxed agent-scope atomics (L1 bypassed), so staleness costs no extra rounds either.
// No lane waits for another: every failed CAS moves the candidate strictly down in key order, every climb strictly too;
// each loop carries a bound (the capacity: no chain is longer) that sets a failure word -> NDT_ERR_INTERNAL.
// The rules of ndt_map.hip hold: wave64, 256-thread blocks, integer atomics only, no kernel waits for another block.
#include "ndt_compact_device.h"
#include "ndt_engine.h"
#include "ndt_map_device.h"

namespace ndt {

namespace {

constexpr uint32_t CC_NONE = 0xffffffffu;   // parent word of a slot that takes no part (empty or ineligible)
constexpr int CC_FOLD_ROUNDS = 2;           // reduce: labels a wave folds before its lanes add for themselves
// words of VoxelMap::cstat as these kernels use them
enum { CCS_FAIL = 0, CCS_LABELLED = 1, CCS_WORDS = 8 };

__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cc_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Climb from x to a node whose parent word read as itself, halving the path on the way.  CC_NONE: the bound ran out.
__device__ __forceinline__ uint32_t cc_find(uint32_t* __restrict__ parent, uint32_t x, long long bound) {
  for (long long it = 0; it < bound; ++it) {
    const uint32_t p = cc_load(parent + x);
    if (p == x) return x;
    const uint32_t g = cc_load(parent + p);
    if (g == p) return p;
    cc_store(parent + x, g);   // (x is no root and never will be again: I2)
    x = g;
  }
  return CC_NONE;
}

__global__ void __launch_bounds__(MAP_THREADS) k_mapcc_init(const unsigned long long* __restrict__ tkeys,
                                                           const int* __restrict__ cnt, long long cap, int min_count,
                                                           uint32_t* __restrict__ parent, int32_t* __restrict__ label) {
  const long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
  if (i >= cap) return;
  parent[i] = tkeys[i] != MAP_EMPTY && cnt[i] >= min_count ? (uint32_t)i : CC_NONE;
  label[i] = -1;
}

// The forward neighbours of slot i's voxel: position n = 14 .. 26 of the 3 x 3 x 3 cube in (k, j, i) order, the centre
// being 13 -- exactly the offsets whose key is larger.  max_s: 1, 2 or 3 (connectivity 6, 18, 26).
__global__ void __launch_bounds__(MAP_THREADS) k_mapcc_link(const unsigned long long* __restrict__ tkeys,
                                                           const int* __restrict__ cnt, long long cap, int min_count, int max_s,
                                                           uint32_t* __restrict__ parent, unsigned long long* __restrict__ cstat) {
  const long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
  if (i >= cap) return;
  const unsigned long long key = tkeys[i];
  if (key == MAP_EMPTY || cnt[i] < min_count) return;
  int v[3];
  map_ijk(key, v);
  const unsigned long long mask = (unsigned long long)(cap - 1);
  bool failed = false;
  for (int n = 14; n < 27; ++n) {
    const int di = n % 3 - 1, dj = (n / 3) % 3 - 1, dk = n / 9 - 1;
    if (abs(di) + abs(dj) + abs(dk) > max_s) continue;
    const int ni = v[0] + di, nj = v[1] + dj, nk = v[2] + dk;
    if (ni <= -MAP_BIAS || ni >= MAP_BIAS || nj <= -MAP_BIAS || nj >= MAP_BIAS || nk >= MAP_BIAS) continue;   // (dk >= 0)
    const long long s = map_find(tkeys, mask, map_key(ni, nj, nk));
    if (s < 0 || cnt[s] < min_count) continue;
    // unite the sets of slot i and slot s
    uint32_t ra = cc_find(parent, (uint32_t)i, cap), rb = cc_find(parent, (uint32_t)s, cap);
    bool done = false;
    for (long long it = 0; it < cap && ra != CC_NONE && rb != CC_NONE; ++it) {
      if (ra == rb) { done = true; break; }
      if (tkeys[ra] > tkeys[rb]) { const uint32_t t = ra; ra = rb; rb = t; }   // rb: the larger key, it goes under ra
      const uint32_t old = atomicCAS(parent + rb, rb, ra);
      if (old == rb) { done = true; break; }
      rb = cc_find(parent, old, cap);   // rb was no root any more: on from what the CAS returned
    }
    if (!done) failed = true;
  }
  if (failed) atomicOr(cstat + CCS_FAIL, 1ull);
}

__global__ void __launch_bounds__(MAP_THREADS) k_mapcc_flatten(long long cap, uint32_t* __restrict__ parent,
                                                              unsigned long long* __restrict__ cstat) {
  const long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
  if (i >= cap) return;
  uint32_t x = cc_load(parent + i);
  if (x == CC_NONE) return;
  // (no hook runs in this launch: the roots are fixed, and whatever another lane has written by now is further up)
  long long it = 0;
  for (; it < cap; ++it) {
    const uint32_t p = cc_load(parent + x);
    if (p == x) break;
    x = p;
  }
  if (it == cap) atomicOr(cstat + CCS_FAIL, 1ull);
  else cc_store(parent + i, x);
}

// the roots among the occupied voxels in key order: output voxel r is slot slots[order[r]]
__global__ void __launch_bounds__(MAP_THREADS) k_mapcc_rootcount(const uint32_t* __restrict__ order, const uint32_t* __restrict__ slots,
                                                                int m, const uint32_t* __restrict__ parent,
                                                                unsigned int* __restrict__ counts) {
  __shared__ unsigned int s_w[MAP_WAVES];
  const int r = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  bool root = false;
  if (r < m) {
    const uint32_t slot = slots[order[r]];
    root = parent[slot] == slot;
  }
  compact_ballot(root, s_w);
  __syncthreads();
  compact_block_count(s_w, counts);
}

// a root's number is its position among the roots; its lane starts the component's record
__global__ void __launch_bounds__(MAP_THREADS) k_mapcc_number(const uint32_t* __restrict__ order, const uint32_t* __restrict__ slots,
                                                             int m, const uint32_t* __restrict__ parent,
                                                             const unsigned long long* __restrict__ tkeys,
                                                             const unsigned int* __restrict__ offsets, unsigned int n_comps,
                                                             int32_t* __restrict__ label, ndt_map_component* __restrict__ comps) {
  __shared__ unsigned int s_w[MAP_WAVES];
  const int r = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  bool root = false;
  uint32_t slot = 0;
  if (r < m) {
    slot = slots[order[r]];
    root = parent[slot] == slot;
  }
  const unsigned long long bal = compact_ballot(root, s_w);
  __syncthreads();
  const unsigned int pos = compact_position(bal, s_w, offsets);
  if (root && pos < n_comps) {
    label[slot] = (int32_t)pos;
    int v[3];
    map_ijk(tkeys[slot], v);
    ndt_map_component c;
    c.root_ijk[0] = v[0]; c.root_ijk[1] = v[1]; c.root_ijk[2] = v[2];
    c.n_voxels = 0;
    c.n_points = 0;
    c.min_ijk[0] = c.min_ijk[1] = c.min_ijk[2] = INT_MAX;
    c.max_ijk[0] = c.max_ijk[1] = c.max_ijk[2] = INT_MIN;
    comps[pos] = c;
  }
}

// Every eligible slot takes its root's label (a root has its own from k_mapcc_number) and brings its voxel to the
// component's record: count, points and box by integer atomics.  The lanes of a wave that share the first remaining
// lane's label are folded into one set of atomics, CC_FOLD_ROUNDS times (a map is mostly one large component); what is
// left adds for itself.  Sums and extrema of integers: the record does not depend on any order.
__global__ void __launch_bounds__(MAP_THREADS) k_mapcc_reduce(const unsigned long long* __restrict__ tkeys, const int* __restrict__ cnt,
                                                             long long cap, const uint32_t* __restrict__ parent,
                                                             int32_t* __restrict__ label, ndt_map_component* __restrict__ comps) {
  const long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
  int lab = -1, c = 0;
  int v[3] = {0, 0, 0};
  if (i < cap) {
    const uint32_t p = parent[i];
    if (p != CC_NONE) {
      lab = label[p];
      if (p != (uint32_t)i) label[i] = lab;
      c = cnt[i];
      map_ijk(tkeys[i], v);
    }
  }
  bool pending = lab >= 0;
#pragma unroll
  for (int round = 0; round < CC_FOLD_ROUNDS; ++round) {
    const unsigned long long bal = __ballot(pending);
    if (bal == 0ull) break;
    const int leader = __ffsll((long long)bal) - 1;
    const int lead_lab = __shfl(lab, leader);
    const bool mine = pending && lab == lead_lab;
    const int nv = wave_sum(mine ? 1 : 0);
    const unsigned long long np = wave_sum_u64(mine ? (unsigned long long)c : 0ull);
    const int lo0 = wave_min(mine ? v[0] : INT_MAX), lo1 = wave_min(mine ? v[1] : INT_MAX), lo2 = wave_min(mine ? v[2] : INT_MAX);
    const int hi0 = wave_max(mine ? v[0] : INT_MIN), hi1 = wave_max(mine ? v[1] : INT_MIN), hi2 = wave_max(mine ? v[2] : INT_MIN);
    if ((int)(threadIdx.x & 63u) == leader) {
      ndt_map_component* q = comps + lead_lab;
      atomicAdd(&q->n_voxels, nv);
      atomicAdd(reinterpret_cast<unsigned long long*>(&q->n_points), np);
      atomicMin(&q->min_ijk[0], lo0); atomicMin(&q->min_ijk[1], lo1); atomicMin(&q->min_ijk[2], lo2);
      atomicMax(&q->max_ijk[0], hi0); atomicMax(&q->max_ijk[1], hi1); atomicMax(&q->max_ijk[2], hi2);
    }
    if (mine) pending = false;
  }
  if (pending) {
    ndt_map_component* q = comps + lab;
    atomicAdd(&q->n_voxels, 1);
    atomicAdd(reinterpret_cast<unsigned long long*>(&q->n_points), (unsigned long long)c);
    atomicMin(&q->min_ijk[0], v[0]); atomicMin(&q->min_ijk[1], v[1]); atomicMin(&q->min_ijk[2], v[2]);
    atomicMax(&q->max_ijk[0], v[0]); atomicMax(&q->max_ijk[1], v[1]); atomicMax(&q->max_ijk[2], v[2]);
  }
}

// output row r = the voxel slots[order[r]]: its ijk and its label (either may be null)
__global__ void __launch_bounds__(MAP_THREADS) k_mapcc_gather(const uint32_t* __restrict__ order, const uint32_t* __restrict__ slots,
                                                             int m, const unsigned long long* __restrict__ tkeys,
                                                             const int32_t* __restrict__ label, int32_t* __restrict__ oijk,
                                                             int32_t* __restrict__ olabel) {
  const int r = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  if (r >= m) return;
  const uint32_t slot = slots[order[r]];
  if (oijk) {
    int v[3];
    map_ijk(tkeys[slot], v);
    oijk[(size_t)r * 3 + 0] = v[0]; oijk[(size_t)r * 3 + 1] = v[1]; oijk[(size_t)r * 3 + 2] = v[2];
  }
  if (olabel) olabel[r] = label[slot];
}

// What one launch of k_mapcc_points knows about its call: the pose as ndt_map_add applies it.
struct LabelPose {
  double R[9], t[3];   // row-major rotation and translation (has_pose)
  int has_pose;
  float inv_leaf;
};

// label (null: an empty map, every point -1) and tkeys of the map; the labelled points are counted in cstat
__global__ void __launch_bounds__(MAP_THREADS) k_mapcc_points(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ z, int n, LabelPose c,
                                                             const unsigned long long* __restrict__ tkeys, unsigned long long mask,
                                                             const int32_t* __restrict__ label, int32_t* __restrict__ out,
                                                             unsigned long long* __restrict__ cstat) {
  __shared__ unsigned long long red[MAP_WAVES];
  const int i = (int)(blockIdx.x * MAP_THREADS + threadIdx.x);
  int lab = -1;
  if (i < n) {
    float a = x[i], b = y[i], d = z[i];
    bool ok = isfinite(a) && isfinite(b) && isfinite(d);
    if (ok && c.has_pose) {   // (launch_transform_append's arithmetic)
      const double pa = (double)a, pb = (double)b, pc = (double)d;
      a = (float)(c.R[0] * pa + c.R[1] * pb + c.R[2] * pc + c.t[0]);
      b = (float)(c.R[3] * pa + c.R[4] * pb + c.R[5] * pc + c.t[1]);
      d = (float)(c.R[6] * pa + c.R[7] * pb + c.R[8] * pc + c.t[2]);
      ok = isfinite(a) && isfinite(b) && isfinite(d);
    }
    if (ok && label) {
      const float fi = floorf(a * c.inv_leaf), fj = floorf(b * c.inv_leaf), fk = floorf(d * c.inv_leaf);   // (k_map_keys' voxel)
      if (fabsf(fi) < MAP_LIMIT && fabsf(fj) < MAP_LIMIT && fabsf(fk) < MAP_LIMIT) {
        const long long s = map_find(tkeys, mask, map_key((int)fi, (int)fj, (int)fk));
        if (s >= 0) lab = label[s];
      }
    }
    out[i] = lab;
  }
  const unsigned long long hits = wave_sum_u64(lab >= 0 ? 1ull : 0ull);
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = hits;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) t += red[w];
    if (t) atomicAdd(cstat + CCS_LABELLED, t);
  }
}

// what stays: an eligible voxel whose component survives, an ineligible one unless they go as well
__device__ __forceinline__ bool cc_stays(int lab, const int32_t* __restrict__ survive, int remove_unlabelled) {
  return lab >= 0 ? survive[lab] != 0 : remove_unlabelled == 0;
}

// Every occupied slot of the old table that stays moves to the new table (map_move_slot); the survivors' ijk box goes to
// tsel (TS_MIN / TS_MAX), their number to *moved (the table's refill counts what it creates).  k_mapstate_crop under the
// survive predicate.
__global__ void __launch_bounds__(MAP_THREADS) k_mapcc_move(MapTable o, const int32_t* __restrict__ label,
                                                           const int32_t* __restrict__ survive, int remove_unlabelled, MapTable t,
                                                           int* __restrict__ stats, int* __restrict__ tsel,
                                                           unsigned long long* __restrict__ moved) {
  __shared__ int box[MAP_WAVES][6], red[MAP_WAVES];
  const long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN}, kept = 0;
  if (i < o.capacity) {
    const unsigned long long key = o.keys[i];
    if (key != MAP_EMPTY && cc_stays(label[i], survive, remove_unlabelled) && map_move_slot(o, i, key, t, stats)) {
      map_ijk(key, mn);
      map_ijk(key, mx);
      kept = 1;
    }
  }
  kept = wave_sum(kept);
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = kept;
  map_box_waves(mn, mx, box);
  __syncthreads();
  map_box_commit(box, tsel + TS_MIN, tsel + TS_MAX);
  if (threadIdx.x == 6) {   // (a thread of the first wave the box leaves idle)
    int v = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) v += red[w];
    if (v) atomicAdd(moved, (unsigned long long)v);
  }
}

}  // namespace

namespace engine {
namespace {

bool cc_params_valid(const ndt_map_components_params* p) {
  return p && (p->connectivity == 6 || p->connectivity == 18 || p->connectivity == 26) && p->min_count >= 1 &&
         p->reserved[0] == 0 && p->reserved[1] == 0;
}

bool cc_filter_valid(const ndt_map_component_filter* f) {
  return f && f->min_voxels >= 1 && f->min_points >= 0 && f->keep_largest >= 0 && f->reserved[0] == 0 && f->reserved[1] == 0 &&
         f->reserved[2] == 0;
}

MapSel cc_sel_all() {   // every occupied voxel, whatever its count
  MapSel sel{};
  sel.min_points = INT_MIN;
  return sel;
}

// after map_refresh_voxel_count with n_voxels > 0: the occupied slots in ascending key order (enqueued)
int cc_export_order(ndt_handle* h, VoxelMap& m, size_t* total, const uint32_t** order, const uint32_t** slots) {
  int rc = map_export_count(h, m, cc_sel_all(), false, total);
  if (rc) return rc;
  if (*total >= (size_t)std::numeric_limits<int>::max()) return fail(h, NDT_ERR_INVALID_ARG, "too many voxels for one labelling");
  return map_export_order(h, m, cc_sel_all(), false, *total, m.mn, m.mx, order, slots);
}

// The labelling of the map under prm stands in m.cclabel / m.cccomps / m.cccomps_h / m.ccinfo when this returns NDT_OK:
// made now, or kept from an earlier call while nothing has changed.
int cc_ensure(ndt_handle* h, const ndt_map_components_params& prm) {
  VoxelMap& m = *h->map;
  settle_discard_keep_grid(h);
  int rc = map_refresh_voxel_count(h, m);
  if (rc) return rc;
  if (m.cc_valid && m.cc_change == m.change && m.cc_connectivity == prm.connectivity && m.cc_min_count == prm.min_count) return NDT_OK;
  m.cc_valid = false;
  m.cccomps_h.clear();
  m.ccinfo = ndt_map_components_info{};
  m.ccinfo.largest = -1;
  if (m.n_voxels > 0) {
    hipStream_t s = h->stream;
    const long long cap = (long long)m.tab.capacity;
    HIP_TRY(h, m.ccparent.ensure((size_t)cap));
    HIP_TRY(h, m.cclabel.ensure((size_t)cap));
    HIP_TRY(h, m.cstat.ensure(CCS_WORDS));
    HIP_TRY(h, m.cstat_h.ensure(CCS_WORDS));
    HIP_TRY(h, hipMemsetAsync(m.cstat.p, 0, CCS_WORDS * sizeof(unsigned long long), s));
    const unsigned slot_blocks = (unsigned)((cap + MAP_THREADS - 1) / MAP_THREADS);
    const int max_s = prm.connectivity == 6 ? 1 : prm.connectivity == 18 ? 2 : 3;
    hipLaunchKernelGGL(k_mapcc_init, dim3(slot_blocks), dim3(MAP_THREADS), 0, s, m.tab.keys, m.tab.cnt, cap, prm.min_count,
                       m.ccparent.p, m.cclabel.p);
    hipLaunchKernelGGL(k_mapcc_link, dim3(slot_blocks), dim3(MAP_THREADS), 0, s, m.tab.keys, m.tab.cnt, cap, prm.min_count, max_s,
                       m.ccparent.p, m.cstat.p);
    hipLaunchKernelGGL(k_mapcc_flatten, dim3(slot_blocks), dim3(MAP_THREADS), 0, s, cap, m.ccparent.p, m.cstat.p);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(m.cstat_h.h, m.cstat.p, CCS_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    size_t total = 0;
    const uint32_t *order = nullptr, *slots = nullptr;
    rc = cc_export_order(h, m, &total, &order, &slots);   // (its count waits for the stream: the failure word is here)
    if (rc) return rc;
    if (m.cstat_h.h[CCS_FAIL] != 0) return fail(h, NDT_ERR_INTERNAL, "voxel map components: a union-find loop ran out of its bound");
    const int nb = (int)((total + MAP_THREADS - 1) / MAP_THREADS);
    rc = compact_scratch(h, nb);
    if (rc) return rc;
    unsigned int* counts = h->compact.counts.p;
    hipLaunchKernelGGL(k_mapcc_rootcount, dim3((unsigned)nb), dim3(MAP_THREADS), 0, s, order, slots, (int)total, m.ccparent.p, counts);
    launch_filter_scan(counts, nb, h->compact.d_total(nb), s);
    size_t n_comps = 0;
    rc = compact_total(h, nb, total, &n_comps);   // the labelling's host wait for C
    if (rc) return rc;
    if (n_comps > 0) {
      HIP_TRY(h, m.cccomps.ensure(n_comps));
      hipLaunchKernelGGL(k_mapcc_number, dim3((unsigned)nb), dim3(MAP_THREADS), 0, s, order, slots, (int)total, m.ccparent.p, m.tab.keys,
                         counts, (unsigned int)n_comps, m.cclabel.p, m.cccomps.p);
      hipLaunchKernelGGL(k_mapcc_reduce, dim3(slot_blocks), dim3(MAP_THREADS), 0, s, m.tab.keys, m.tab.cnt, cap, m.ccparent.p,
                         m.cclabel.p, m.cccomps.p);
      HIP_TRY(h, hipGetLastError());
      m.cccomps_h.resize(n_comps);
      HIP_TRY(h, hipMemcpyAsync(m.cccomps_h.data(), m.cccomps.p, n_comps * sizeof(ndt_map_component), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    ndt_map_components_info& info = m.ccinfo;
    info.n_components = (int64_t)n_comps;
    for (size_t c = 0; c < n_comps; ++c) {
      const ndt_map_component& q = m.cccomps_h[c];
      info.n_voxels_labelled += q.n_voxels;
      if (info.largest < 0 || q.n_voxels > info.largest_n_voxels) {
        info.largest = (int64_t)c;
        info.largest_n_voxels = q.n_voxels;
        info.largest_n_points = q.n_points;
      }
    }
    info.n_voxels_unlabelled = m.n_voxels - info.n_voxels_labelled;
  }
  m.cc_valid = true;
  m.cc_change = m.change;
  m.cc_connectivity = prm.connectivity;
  m.cc_min_count = prm.min_count;
  return NDT_OK;
}

// the labels of every occupied voxel in export order into device arrays (either may be null); *n_out = the voxels
int cc_export_labels(ndt_handle* h, const ndt_map_components_params& prm, int32_t* d_ijk, int32_t* d_label, size_t cap, size_t* n_out) {
  VoxelMap& m = *h->map;
  int rc = cc_ensure(h, prm);
  if (rc) return rc;
  *n_out = (size_t)m.n_voxels;
  const size_t w = std::min((size_t)m.n_voxels, cap);
  if (w == 0 || !(d_ijk || d_label)) return NDT_OK;
  size_t total = 0;
  const uint32_t *order = nullptr, *slots = nullptr;
  rc = cc_export_order(h, m, &total, &order, &slots);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mapcc_gather, dim3((unsigned)((w + MAP_THREADS - 1) / MAP_THREADS)), dim3(MAP_THREADS), 0, h->stream, order, slots,
                     (int)w, m.tab.keys, m.cclabel.p, d_ijk, d_label);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NDT_OK;
}

// n > 0 points in device memory under an optional pose, behind the argument checks
int cc_label_points(ndt_handle* h, const ndt_map_components_params& prm, const float* dx, const float* dy, const float* dz, size_t n,
                    const double* pose16, int32_t* d_out, int64_t* n_labelled) {
  VoxelMap& m = *h->map;
  if (n > (size_t)std::numeric_limits<int>::max() / 2) return fail(h, NDT_ERR_INVALID_ARG, "cloud too large");
  int rc = cc_ensure(h, prm);
  if (rc) return rc;
  LabelPose c{};
  c.has_pose = pose16 ? 1 : 0;
  c.inv_leaf = m.inv_leaf;
  if (pose16) {   // (launch_transform_append's matrix)
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) c.R[3 * i + j] = pose16[4 * j + i];
      c.t[i] = pose16[12 + i];
    }
  }
  hipStream_t s = h->stream;
  HIP_TRY(h, m.cstat.ensure(CCS_WORDS));
  HIP_TRY(h, m.cstat_h.ensure(CCS_WORDS));
  HIP_TRY(h, hipMemsetAsync(m.cstat.p, 0, CCS_WORDS * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_mapcc_points, dim3((unsigned)((n + MAP_THREADS - 1) / MAP_THREADS)), dim3(MAP_THREADS), 0, s, dx, dy, dz, (int)n, c,
                     m.tab.keys, (unsigned long long)(m.tab.capacity - 1), m.n_voxels > 0 ? m.cclabel.p : nullptr, d_out, m.cstat.p);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(m.cstat_h.h, m.cstat.p, CCS_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  if (n_labelled) *n_labelled = (int64_t)m.cstat_h.h[CCS_LABELLED];
  return NDT_OK;
}

int cc_remove(ndt_handle* h, const ndt_map_components_params& prm, const ndt_map_component_filter& f,
              ndt_map_remove_components_result* out) {
  VoxelMap& m = *h->map;
  int rc = cc_ensure(h, prm);
  if (rc) return rc;
  const size_t C = m.cccomps_h.size();
  // which components survive: decided on the host from the C records
  std::vector<int32_t> survive(C, 1);
  if (f.keep_largest > 0 && (size_t)f.keep_largest < C) {
    std::vector<uint32_t> rank(C);
    for (size_t c = 0; c < C; ++c) rank[c] = (uint32_t)c;
    std::stable_sort(rank.begin(), rank.end(), [&](uint32_t a, uint32_t b) { return m.cccomps_h[a].n_voxels > m.cccomps_h[b].n_voxels; });
    for (size_t r = (size_t)f.keep_largest; r < C; ++r) survive[rank[r]] = 0;
  }
  int64_t comps_removed = 0, removed = 0, pts_removed = 0, pts_labelled = 0;
  for (size_t c = 0; c < C; ++c) {
    const ndt_map_component& q = m.cccomps_h[c];
    if (q.n_voxels < f.min_voxels || q.n_points < f.min_points) survive[c] = 0;
    pts_labelled += q.n_points;
    if (!survive[c]) { ++comps_removed; removed += q.n_voxels; pts_removed += q.n_points; }
  }
  if (f.remove_unlabelled) {
    removed += m.ccinfo.n_voxels_unlabelled;
    pts_removed += m.n_points - pts_labelled;
  }
  if (out) {
    *out = ndt_map_remove_components_result{};
    out->n_components = (int64_t)C;
    out->n_components_removed = comps_removed;
    out->n_removed = removed;
    out->n_points_removed = pts_removed;
  }
  if (f.dry_run || removed == 0) return NDT_OK;   // the table is as it was

  hipStream_t s = h->stream;
  HIP_TRY(h, m.ccsurvive.ensure(std::max<size_t>(C, 1)));
  if (C) HIP_TRY(h, hipMemcpy(m.ccsurvive.p, survive.data(), C * sizeof(int32_t), hipMemcpyHostToDevice));
  const int64_t kept = m.n_voxels - removed;
  const int64_t new_cap = std::max(map_pow2_at_least(2 * kept), m.reset_capacity);
  const unsigned slot_blocks = (unsigned)((m.tab.capacity + MAP_THREADS - 1) / MAP_THREADS);
  // The table is replaced the one way a table is (map_grow_table with a refill -> map_replace_table): the move counts the
  // voxels it creates, their tight ijk box comes back through tsel under the replacement's own wait.
  const MapRefill refill{"voxel map remove components: ", [&](const MapTable& fresh) -> int {
    HIP_TRY(h, hipMemcpyAsync(m.tsel.p, m.tsel_h.h + TS_WORDS, TS_WORDS * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_mapcc_move, dim3(slot_blocks), dim3(MAP_THREADS), 0, s, m.tab, m.cclabel.p, m.ccsurvive.p, f.remove_unlabelled,
                       fresh, m.stats.p, m.tsel.p, m.nvox.p + 1);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(m.tsel_h.h, m.tsel.p, TS_WORDS * sizeof(int), hipMemcpyDeviceToHost, s));
    return NDT_OK;
  }};
  rc = map_grow_table(h, m, new_cap, &refill);
  if (rc) return rc;
  if (m.n_voxels != kept) return fail(h, NDT_ERR_INTERNAL, "voxel map remove components: the move kept another number of voxels than the labels say");
  if (kept > 0)
    for (int a = 0; a < 3; ++a) { m.mn[a] = m.tsel_h.h[TS_MIN + a]; m.mx[a] = m.tsel_h.h[TS_MAX + a]; }
  m.n_points -= pts_removed;
  m.cc_valid = false;   // (the labels were the old table's)
  return NDT_OK;
}

// what every call does once its arguments have passed: the device, the map
int cc_enter(ndt_handle* h) {
  const int rc = bind_device(h);
  if (rc) return rc;
  if (!h->map) return no_map(h);
  return NDT_OK;
}

}  // namespace
}  // namespace engine
}  // namespace ndt

extern "C" {

void ndt_map_components_default_params(ndt_map_components_params* p) {
  if (!p) return;
  *p = ndt_map_components_params{};
  p->connectivity = 26;
  p->min_count = 1;
}

void ndt_map_component_filter_default_params(ndt_map_component_filter* f) {
  if (!f) return;
  *f = ndt_map_component_filter{};
  f->min_voxels = 1;
}

int ndt_map_components(ndt_handle* h, const ndt_map_components_params* prm, ndt_map_components_info* info) {
  if (!h || !cc_params_valid(prm)) return NDT_ERR_INVALID_ARG;
  int rc = cc_enter(h);
  if (rc) return rc;
  rc = cc_ensure(h, *prm);
  if (rc) return rc;
  if (info) *info = h->map->ccinfo;
  return NDT_OK;
}

int ndt_map_export_components(ndt_handle* h, const ndt_map_components_params* prm, ndt_map_component* comps, size_t cap, size_t* n_out) {
  if (!h || !cc_params_valid(prm) || !n_out || (!comps && cap)) return NDT_ERR_INVALID_ARG;
  int rc = cc_enter(h);
  if (rc) return rc;
  rc = cc_ensure(h, *prm);
  if (rc) return rc;
  const std::vector<ndt_map_component>& c = h->map->cccomps_h;
  *n_out = c.size();
  const size_t w = std::min(c.size(), cap);
  if (w) std::memcpy(comps, c.data(), w * sizeof(ndt_map_component));
  if (c.size() > cap) return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(c.size()) + " components");
  return NDT_OK;
}

int ndt_map_export_labels_device(ndt_handle* h, const ndt_map_components_params* prm, int32_t* ijk, int32_t* label, size_t cap,
                                 size_t* n_out) {
  if (!h || !cc_params_valid(prm) || !n_out) return NDT_ERR_INVALID_ARG;
  int rc = cc_enter(h);
  if (rc) return rc;
  size_t total = 0;
  rc = cc_export_labels(h, *prm, ijk, label, cap, &total);
  if (rc) return rc;
  *n_out = total;
  if (total > cap) return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(total) + " voxels");
  return NDT_OK;
}

int ndt_map_export_labels(ndt_handle* h, const ndt_map_components_params* prm, int32_t* ijk, int32_t* label, size_t cap, size_t* n_out) {
  if (!h || !cc_params_valid(prm) || !n_out) return NDT_ERR_INVALID_ARG;
  int rc = cc_enter(h);
  if (rc) return rc;
  VoxelMap& m = *h->map;
  settle_discard_keep_grid(h);
  rc = map_refresh_voxel_count(h, m);
  if (rc) return rc;
  const size_t w = std::min((size_t)m.n_voxels, cap);
  if (w && ijk) HIP_TRY(h, m.xijk.ensure(3 * w));
  if (w && label) HIP_TRY(h, m.xcnt.ensure(w));
  size_t total = 0;
  rc = cc_export_labels(h, *prm, ijk && w ? m.xijk.p : nullptr, label && w ? m.xcnt.p : nullptr, w, &total);
  if (rc) return rc;
  *n_out = total;
  const size_t got = std::min(total, w);
  if (got && ijk) HIP_TRY(h, hipMemcpy(ijk, m.xijk.p, 3 * got * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (got && label) HIP_TRY(h, hipMemcpy(label, m.xcnt.p, got * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (total > cap) return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(total) + " voxels");
  return NDT_OK;
}

int ndt_map_label_points_device(ndt_handle* h, const ndt_map_components_params* prm, const float* dx, const float* dy, const float* dz,
                                size_t n, const double* pose16, int32_t* d_label_out, int64_t* n_labelled) {
  if (!h || !cc_params_valid(prm) || ((!dx || !dy || !dz || !d_label_out) && n) || (pose16 && !pose_finite(pose16)))
    return NDT_ERR_INVALID_ARG;
  int rc = cc_enter(h);
  if (rc) return rc;
  if (n == 0) {
    if (n_labelled) *n_labelled = 0;
    return NDT_OK;
  }
  return cc_label_points(h, *prm, dx, dy, dz, n, pose16, d_label_out, n_labelled);
}

int ndt_map_label_points(ndt_handle* h, const ndt_map_components_params* prm, const float* xyz, size_t n, size_t stride_bytes,
                         const double* pose16, int32_t* label_out, int64_t* n_labelled) {
  if (!h || !cc_params_valid(prm) || ((!xyz || !label_out) && n) || !layout_valid(stride_bytes, -1) ||
      (pose16 && !pose_finite(pose16)))
    return NDT_ERR_INVALID_ARG;
  int rc = cc_enter(h);
  if (rc) return rc;
  if (n == 0) {
    if (n_labelled) *n_labelled = 0;
    return NDT_OK;
  }
  VoxelMap& m = *h->map;
  settle_discard_keep_grid(h);
  rc = upload_soa(h, h->lane_t, h->stream, xyz, nullptr, nullptr, nullptr, n, stride_bytes, m.ux, m.uy, m.uz, true);
  if (rc) return rc;
  HIP_TRY(h, m.xcnt.ensure(n));
  rc = cc_label_points(h, *prm, m.ux.p, m.uy.p, m.uz.p, n, pose16, m.xcnt.p, n_labelled);
  if (rc) return rc;
  HIP_TRY(h, hipMemcpy(label_out, m.xcnt.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return NDT_OK;
}

int ndt_map_remove_components(ndt_handle* h, const ndt_map_components_params* prm, const ndt_map_component_filter* filter,
                              ndt_map_remove_components_result* out) {
  if (!h || !cc_params_valid(prm) || !cc_filter_valid(filter)) return NDT_ERR_INVALID_ARG;
  int rc = cc_enter(h);
  if (rc) return rc;
  return cc_remove(h, *prm, *filter, out);
}

}  // extern "C"
