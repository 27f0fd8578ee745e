// ndt_engine.h -- the engine's handle and the functions its translation units share (internal; the public
// boundary is include/ndt_hip.h).  Round 5 split the former ndt_api.hip along these lines:
//   ndt_handle.hip     handle life cycle, parameters, reducers' entry points, timing, test seams
//   ndt_handoff.hip    host hand-off (repack + pull kernels), the target voxel-grid build's orchestration, grid accessors
//   ndt_evaluate.hip   derivative evaluations (ordinary, pre-launched, batched), align, scoring
//   ndt_keyframes.hip  multi-grid targets, the device-resident keyframe archive, voxel downsample
//   ndt_sort.hip       the keyed sort every subsystem shares: radix sort kernels, plan writer, sort call, run-search scratch
//   ndt_point_scores.hip  per-point scores and the score-based source filter; the engine's one scan of block counts and
//                      the host side of every compaction (the device side: ndt_compact_device.h)
//   ndt_map.hip        the sparse voxel map accumulated scan by scan (ndt_map_*), its kernels included
//   ndt_map_state.hip  the map's crop, full-state export / import and merge (k_mapstate_* kernels)
//   ndt_map_repose.hip the map moved by a pose, and records merged under one (k_maprepose_* kernels)
//   ndt_map_levels.hip the map at leaf * 2^L derived from its own sums and cached beside it, a level as the target, the map
//                      coarsened to a level, coarse-to-fine align over the levels (k_maplevel_* kernels)
//   ndt_d2d.hip        distribution-to-distribution registration: a source of Gaussians from map records, its evaluation
//                      and align against the target's leaves (k_d2d_* kernels)
//   ndt_ct.hip         continuous-time registration: per-point times of the point source, the evaluation with one pose per
//                      point, its align and the deskewed scan under a result (k_ct_* kernels)
//   ndt_gicp.hip       generalised ICP: the exact k nearest neighbours of every point of a cloud, the point covariances made
//                      from them, the frozen nearest-point pairs, the plane-to-plane evaluation over them and the two-level
//                      align (k_gicp_* kernels); the index it searches is the fitness index (ndt_fitness.hip, ndt_fit_device.h)
//   ndt_vgicp.hip      voxelised GICP: the target's point covariances aggregated into the target's leaves, the evaluation
//                      of a source point against up to seven of those voxels and the one-level align (k_vgicp_* kernels)
//   ndt_eval_rows.hip  what those evaluations share behind their kernels: the fixed-order sum of block rows, the host
//                      driver, the support check, the finished-words repack, the align wrapper
//   ndt_scan_context.hip  Scan Context place recognition: a scan's rings x sectors descriptor, the descriptor bank beside
//                      the keyframe archive and the all-shifts match against it (k_sc_* kernels)
//   ndt_map_carve.hip  free-space carving of the map: voxels that a scan's rays pass through go (k_mapcarve_* kernels)
//   ndt_deskew.hip     motion compensation of a scan along a pose trajectory + the acquisition filter (its kernels included)
//   ndt_unproject.hip  a lidar range image -> points through the scan model's tables, fused with that filter and deskew
// One handle = one engine instance = one HIP stream on one gfx950 device; it owns every device allocation.  There is no
// CPU path: without a device every compute call fails with NDT_ERR_NO_DEVICE.
#pragma once

#include <immintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <random>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <limits>
#include <string>
#include <thread>
#include <map>
#include <unordered_map>
#include <vector>

#include "../../include/ndt_hip.h"
#include "ndt_comm.h"
#include "ndt_host_cloud.h"
#include "ndt_keepwarm.h"
#include "ndt_kernels.h"
#include "ndt_newton.h"
#include "ndt_packets.h"
#include "ndt_repack_pool.h"
#include "ndt_target_state.h"
#include "ndt_tuning.h"

using namespace ndt;

namespace ndt {

struct MapSel;   // ndt_map_device.h
namespace traj {
struct KnotRow;  // ndt_trajectory.h
}

namespace engine {

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + n / 8 + 64;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// The dense cell -> leaf index with four readable ints in front of the first cell and behind the last: the 27-cell
// neighbourhoods load a row of three x-adjacent cells with ONE 12-byte load, which at the ends of the grid starts one
// or two ints outside it (those lanes are masked, the bytes only have to be mapped).  Same member names as DevBuf.
struct IndexGrid {
  DevBuf<int> raw;
  int* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    p = nullptr;
    cap = 0;
    hipError_t e = raw.ensure(n + 8);
    if (e == hipSuccess) { p = raw.p + 4; cap = raw.cap - 8; }
    return e;
  }
  void release() { raw.release(); p = nullptr; cap = 0; }
};

template <typename T>
struct PinBuf {  // pinned, device-mapped host memory
  T* h = nullptr;
  T* d = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&h), n * sizeof(T), hipHostMallocMapped);
    if (e != hipSuccess) { h = nullptr; return e; }
    e = hipHostGetDevicePointer(reinterpret_cast<void**>(&d), h, 0);
    if (e != hipSuccess) { (void)hipHostFree(h); h = nullptr; return e; }
    cap = n;
    return hipSuccess;
  }
  void release() {
    if (h) (void)hipHostFree(h);
    h = nullptr; d = nullptr; cap = 0;
  }
};

// One logged evaluation (ndt_debug_eval_log, a test seam; not in the public header): what went to the device, the raw 32
// words that came back -- after the cross-rank sum, before finish_eval (ridge / regularisation) -- and the launch that
// made them.  A batched launch logs one entry per pose (same `launch`, k = 0 .. K - 1).  The Python binding reads the
// entries with a matching NumPy dtype (EVAL_LOG_DTYPE, slam-sam_amd/__init__.py).
struct EvalLogEntry {
  double pose6[6];
  double words[EV_WORDS];
  float T[16];
  int64_t launch;      // launches logged before this one
  int k, K;            // pose of the launch, poses of the launch
  int need_h, score_only;
  int prelaunched;     // served by a kernel enqueued before its pose was known (the mailbox)
  int pad;
  DerivLaunchPlan plan;
};
static_assert(sizeof(EvalLogEntry) == 464, "EvalLogEntry layout is read from Python");

// The five arrays of one stable radix sort of (key, index) pairs (ndt_sort.hip): the keys go into `keys`, sort_keyed
// ping-pongs between the two pairs of arrays and says where the result is.  Three instances, each with its own memory: the
// handle's (the build, the downsample, the voxel map, ndt_debug_sort_pairs), the fitness index's and the source ordering's.
struct SortScratch {
  DevBuf<uint32_t> keys, vals, keys2, vals2;
  DevBuf<char> tmp;                  // sort_temp_bytes(n): tile histograms of the digit in flight + bin totals
  hipError_t ensure(size_t n);       // n pairs
  void release() { keys.release(); vals.release(); keys2.release(); vals2.release(); tmp.release(); }
};

// Geometry of the point-level nearest-neighbour index (ndt_fitness.hip): cells of edge `c` on the bounding box of the
// target's finite points, cell (i, j, k) = floor((p - lo) * inv_c) per axis in f32, key i + dims0 * (j + dims1 * k).
struct FitGeom {
  float lo[3];
  float c, inv_c;
  int dims[3];
  uint32_t ncells;     // dims0 * dims1 * dims2 (< 2^30); also the key of a non-finite point
  uint32_t hash_mask;  // open-addressing table of hash_mask + 1 slots
  int n_finite;
};

// The index itself (built lazily by the first fitness call after the target changed; owns every buffer it uses --
// the grid build's scratch is reused by ndt_voxel_downsample* and by builds).
struct FitIndex {
  uint64_t gen = 0;                  // TargetState::gen() of the target it indexes
  bool valid = false;
  FitGeom g{};
  DevBuf<float> pts;                 // the finite target points as float4, sorted by cell (stable)
  DevBuf<uint32_t> tab;              // hash table, 4 words per slot: {cell key, first point, end point, 0}
  SortScratch sort;
  DevBuf<BuildGeom> plan;            // its sort plan (sort_put_plan)
  DevBuf<float> bslab;               // per-block bounds {min xyz, max xyz}
  DevBuf<int> cslab;                 // ... and finite counts
  PinBuf<float> bslab_h;
  PinBuf<int> cslab_h;
  // query
  DevBuf<float> dist;                // K x n_src: d^2 (NaN / +INF as the C-ABI documents)
  DevBuf<int> work;                  // [0] unresolved entries, then the entries (k * n_src + i)
  DevBuf<float> poses;               // K x 12 floats {R row-major, t}
  DevBuf<double> slab;               // K x blocks x 3: {sum d^2, inliers, finite points}
  PinBuf<double> slab_h;
  void release() {
    pts.release(); tab.release(); sort.release(); plan.release(); bslab.release(); cslab.release(); bslab_h.release(); cslab_h.release(); dist.release(); work.release();
    poses.release(); slab.release(); slab_h.release();
    valid = false;
  }
};

// Scratch of a stream compaction (ndt_compact_device.h), one per handle: ndt_filter_source*, ndt_deskew* and
// ndt_unproject* are serial on a handle and awaited before they return.  compact_scratch / compact_total use it.
struct CompactBufs {
  DevBuf<unsigned int> counts;       // nb block counts / offsets, their sum, then the total the scan writes: nb + 2 words
  PinBuf<unsigned int> total_h;      // ... and where the host reads it
  unsigned int* d_total(int nb) const { return counts.p + nb + 1; }
  void release() { counts.release(); total_h.release(); }
};

// The knot table of a trajectory on the device, one per handle (knots_upload; ndt_deskew* and ndt_unproject* read it)
struct KnotTable {
  DevBuf<double> tab;                // <= 64 rows of 12 doubles (traj::KnotRow)
  PinBuf<double> tab_h;              // its pinned staging
  void release() { tab.release(); tab_h.release(); }
};

// Scratch of the per-point scoring calls: the host forms' device-side outputs, the filter's predicate values and (host
// form) compacted output.  Kept between calls.
struct PointScoreBufs {
  DevBuf<double> score, best;
  DevBuf<int> npairs, index;
  DevBuf<long long> cell;
  DevBuf<float> out;                 // [x | y | z] of the selected points
  void release() { score.release(); best.release(); npairs.release(); index.release(); cell.release(); out.release(); }
};

// Scratch of the deskew calls' host forms (ndt_deskew.hip), kept between calls: the raw scan and the result on the
// device and a pinned staging.
struct DeskewBufs {
  DevBuf<float> in;                  // [x | y | z | t | intensity] of a host scan
  DevBuf<float> out;                 // [x | y | z | intensity] of the result
  DevBuf<int> index;
  PinBuf<float> stage;               // the host scan on its way up, the result on its way down
  void release() { in.release(); out.release(); index.release(); stage.release(); }
};

// The scan model of ndt_scan_model_set and the scratch of the unprojection calls (ndt_unproject.hip), kept between
// calls: the model's tables, and for the host and keyframe forms the raw range image and the result on the device and a
// pinned staging.
struct ScanModelBufs {
  int n_cols = 0, n_rows = 0;        // 0, 0: no model set
  DevBuf<float> dir;                 // [x1 | y1 | z1], n_cols * n_rows floats each, pixel col * n_rows + row
  DevBuf<float> off;                 // [x2 | y2 | z2], n_cols floats each
  DevBuf<uint32_t> in;               // a host range image: [range_mm (n words) | col_t (n_cols words) | reflectivity (n bytes)]
  DevBuf<float> out;                 // [x | y | z | intensity | t] of the result
  DevBuf<int> index;
  PinBuf<uint32_t> stage;            // the range image on its way up, the result on its way down
  void release() {
    n_cols = n_rows = 0;
    dir.release(); off.release(); in.release(); out.release(); index.release(); stage.release();
  }
};

// The packet format of ndt_packet_format_set, the frame in progress and the scratch of the packet calls (ndt_packets.hip):
// the accepted packets in a pinned staging and in the device packet buffer (slot k of both = the k-th accepted packet),
// the column table on its way up, and signal / nir of the decoded image for the forms that unproject.
struct PacketBufs {
  pkt::Pass pass;                    // pass.f.profile < 0: no format set
  PinBuf<uint32_t> stage;            // capacity * slot bytes
  DevBuf<uint32_t> dev;              // the packed packet buffer
  PinBuf<uint32_t> cols_h;           // [col_src (n_cols int32) | col_t (n_cols floats)]
  DevBuf<int32_t> col_src;           // n_cols
  DevBuf<uint16_t> sig, nir;         // n_cols * n_rows each: the decoded image's
  DevBuf<uint16_t> sig_out, nir_out; // ... and the selected points' (host forms)
  PinBuf<uint16_t> back;             // ... on their way down
  void drop() { pass.f = pkt::Format{}; pass.begin(pass.f); }
  void release() {
    drop();
    stage.release(); dev.release(); cols_h.release(); col_src.release(); sig.release(); nir.release(); sig_out.release();
    nir_out.release(); back.release();
  }
};

// The distribution source of the D2D registration and what its evaluations need (ndt_d2d.hip).  The records are kept as
// handed over: the Gaussians are derived from them under the handle's leaf rule and re-derived when that rule has changed
// (d2d_source_fresh).  The target's leaves as the kernel reads them (mean 3 + cov 6 per leaf slot) are gathered from
// `stats` by the first D2D evaluation after a target was published; target_retire and target_drop invalidate them.
struct D2dBufs {
  DevBuf<int32_t> rcount;            // the records: counts ...
  DevBuf<double> rmom;               // ... and nine f64 sums each
  size_t n_records = 0;
  bool have = false;                 // a distribution source is set
  int rule_min_pts = 0, rule_cov_mode = 0;   // the leaf rule the Gaussians below were derived under
  double rule_eig = 0.0;
  DevBuf<double> gauss;              // the accepted Gaussians in input order: {mean xyz, cov xx xy xz yy yz zz}
  DevBuf<int32_t> gcount, gindex;    // ... their counts and their records
  size_t n_accepted = 0;
  DevBuf<VoxelRecord> frec;          // finalize_leaf's outputs for the records (scratch of the derivation)
  DevBuf<float> fcent;
  DevBuf<LeafStats> fstats;
  DevBuf<int> fcell;                 // record r -> r if it was accepted, else -1
  DevBuf<int> bad;                   // the device setter's argument check
  PinBuf<int> bad_h;
  DevBuf<double> tleaf;              // the target's leaves, 9 doubles per slot
  uint64_t tleaf_gen = 0;            // TargetState::gen() of the target they were gathered from
  bool tleaf_valid = false;
  void release() {
    rcount.release(); rmom.release(); gauss.release(); gcount.release(); gindex.release(); frec.release(); fcent.release();
    fstats.release(); fcell.release(); bad.release(); bad_h.release(); tleaf.release();
    n_records = n_accepted = 0;
    have = tleaf_valid = false;
  }
};

// The times of the point source for the continuous-time calls (ndt_ct.hip) and their scratch.  The times belong to the
// source they were set behind: every call that replaces or re-declares the source sets n back to 0.
struct CtBufs {
  DevBuf<float> alpha;               // one factor per source point, in the source's order
  size_t n = 0;                      // times attached (== n_src), 0 = none
  DevBuf<float> xyz;                 // [x | y | z] of ndt_transform_source_ct's host form
  void release() {
    alpha.release(); xyz.release();
    n = 0;
  }
};

// GICP (ndt_gicp.hip).  One cloud's side: the neighbour lists and the covariances derived from them, cached until the cloud
// or the rule (k, distance cap, epsilon) changes.  The source's go with every call that replaces or re-declares the source
// (the list the CT times follow), the target's are tagged with TargetState::gen() like FitIndex.
struct GicpCloud {
  bool valid = false;
  uint64_t gen = 0;                  // target side: TargetState::gen() of the target they were derived from
  size_t n = 0;                      // points of the cloud, rows of everything below (input order)
  int k = 0;                         // row length of nbr
  int64_t n_without = 0;             // points without a covariance
  DevBuf<int32_t> nbr, nfound;       // n x k neighbour indices (-1 padded), neighbours found
  DevBuf<double> mean, raw;          // n x 3 neighbourhood mean, n x 6 raw covariance (NaN rows without a covariance)
  DevBuf<double> gauss;              // n x 9 as the evaluation reads it: {the point itself x y z, regularised cov xx xy xz yy yz zz}
  void release() { nbr.release(); nfound.release(); mean.release(); raw.release(); gauss.release(); valid = false; n = 0; }
};
struct GicpBufs {
  ndt_gicp_params prm{20, INFINITY, 1e-3, 5.0, 1e-4, 64, 20};
  GicpCloud src, tgt;
  FitIndex sidx;                     // the source's own point index (the target's is the handle's `fit`)
  DevBuf<int> work;                  // [0] unresolved queries of a search's pass 1, then their indices; [1 + n]: points without a covariance
  PinBuf<int> work_h;
  // the frozen pairs: per source point the target point's input index (-1: none) and the f32 d^2
  DevBuf<int32_t> pair;
  DevBuf<float> pd2;
  bool pairs_valid = false;
  uint64_t pairs_gen = 0;            // TargetState::gen() of the target they point into
  int64_t n_pairs = 0;
  void drop_pairs() { pairs_valid = false; n_pairs = 0; }
  void drop_source() { src.valid = false; sidx.valid = false; drop_pairs(); }
  void release() { src.release(); tgt.release(); sidx.release(); work.release(); work_h.release(); pair.release(); pd2.release(); drop_pairs(); }
};

// Voxelised GICP (ndt_vgicp.hip): per leaf slot of the target the mean of its points and the mean of their GICP
// covariances, derived lazily from GicpBufs::tgt and cached until the target (gen, target_retire / target_drop) or the
// covariance rule (ndt_gicp_set_params) changes.  The source side is GicpBufs::src.
struct VgicpBufs {
  bool valid = false;
  uint64_t gen = 0;                  // TargetState::gen() of the target the table was derived from
  int n_slots = 0;                   // rows of the table (leaf slots, rejected leaves included: those never pair)
  int64_t n_voxels = 0, n_points = 0;   // leaves with N >= 1, sum of N
  DevBuf<double> table;              // n_slots x 9 in d2d_pair's target layout {mean 3, cov xx xy xz yy yz zz}; NaN rows for N = 0
  DevBuf<int32_t> count;             // N per slot
  SortScratch sort;                  // (leaf slot, point index) pairs of the derivation ...
  DevBuf<BuildGeom> plan;            // ... and their sort plan
  void release() { table.release(); count.release(); sort.release(); plan.release(); valid = false; }
};

// The rows of a lane-per-item evaluation (lane_eval_rows, ndt_eval_rows.hip).  One instance serves D2D, CT, GICP and VGICP: each
// evaluation is awaited before it returns.
struct EvalRowBufs {
  DevBuf<double> rows, out;          // per-block rows of K poses, their K x EV_WORDS sums
  PinBuf<double> out_h;
  void release() { rows.release(); out.release(); out_h.release(); }
};

// Scan Context (ndt_scan_context.hip): the parameters, the sector table they imply, the scratch of a descriptor call and
// the descriptor bank -- slots of n_rings x n_sectors floats in one device array, `ids` naming the slot of every entry
// (ascending ids: the order of a match's outputs).  ndt_keyframe_erase leaves the bank alone; a parameter change clears it.
struct ScanContextBufs {
  ndt_scan_context_params prm{20, 60, 80.0f, 1.0f, 2.0f, 1};
  bool table_valid = false;          // `dir` holds the table of prm.n_sectors
  DevBuf<float> dir;                 // S x 2: ndt_scan_context_sector_table's floats
  DevBuf<uint32_t> acc;              // [desc bits (R x S) | counts (R x S)]: what the blocks' LDS copies merge into
  DevBuf<float> ux, uy, uz;          // a host scan on the device
  DevBuf<float> desc;                // a descriptor on its way to the host, or a query on its way up
  DevBuf<int32_t> count;
  DevBuf<float> bank;                // bank_slots() slots of bins() floats
  std::map<int64_t, int> ids;        // entry -> slot
  std::vector<int> free_slots;
  DevBuf<int> order;                 // the slots in ascending id order, as the match kernel reads them
  bool order_valid = false;
  DevBuf<double> mdist;              // a match's outputs, one per entry
  DevBuf<int32_t> mshift, mcols;
  size_t bins() const { return (size_t)prm.n_rings * (size_t)prm.n_sectors; }
  size_t bank_slots() const { return bank.cap / bins(); }
  void clear_bank() { ids.clear(); free_slots.clear(); order_valid = false; }
  void release() {
    dir.release(); acc.release(); ux.release(); uy.release(); uz.release(); desc.release(); count.release(); bank.release();
    order.release(); mdist.release(); mshift.release(); mcols.release();
    table_valid = false;
    clear_bank();
  }
};

// The voxel map's table, as its kernels take it (by value) and as growth, crop and carve replace it (map_replace_table).
struct MapTable {
  unsigned long long* keys = nullptr;  // capacity words, ~0 = empty
  float4* sums = nullptr;              // capacity
  int* cnt = nullptr;                  // capacity
  double* mom = nullptr;               // capacity x 9 doubles; allocated only with moments on
  int64_t capacity = 0;
};
void map_free_table(MapTable& t);      // ndt_map.hip: frees what t holds and leaves it empty

// The sparse voxel map of ndt_map_* (ndt_map.hip): an open-addressing table in HBM keyed by the 63-bit voxel key
// (k, j, i), the table position being the voxel's slot -- float sums {x, y, z, intensity} and an int32 count per slot,
// and with moments on (ndt_map_enable_moments) the nine f64 sums of the target build {x, y, z, xx, xy, xz, yy, yz, zz}:
// 28 or 100 bytes per slot.
// The host keeps the counters it knows when an add's range check returns; the number of voxels is counted on the
// device by the insert launch and fetched under the next host wait (nvox_stale).
struct VoxelMap {
  float leaf = 0.0f, inv_leaf = 0.0f;
  int with_intensity = 0;
  MapTable tab;
  bool moments = false;
  int64_t reset_capacity = 0;          // the capacity ndt_map_reset gave it: a crop never shrinks the table below it
  int64_t n_voxels = 0, n_points = 0, n_dropped = 0, n_adds = 0, n_grows = 0;
  int mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  bool nvox_stale = false;             // the device's voxel counter is ahead of n_voxels
  // Levels (ndt_map_levels.hip).  The map: `change` goes up wherever the table's content changes (add, import, every
  // table replacement, enable_moments).  A level (ndt_handle::map_level): `derived_at` is the map's `change` it was
  // derived at, `lchild` its derivation's table position per ordered fine voxel.
  uint64_t change = 0, derived_at = 0;
  DevBuf<uint32_t> lchild;
  DevBuf<unsigned long long> pkey;     // the batch's voxel keys
  DevBuf<float> px, py, pz;            // the batch moved by its pose
  DevBuf<float> ux, uy, uz, ui;        // a host batch on the device
  DevBuf<int> stats;                   // per add: {finite, out of range, min ijk, max ijk, probe failures}
  DevBuf<unsigned long long> nvox;     // occupied slots (cumulative); [1]: those a re-pose creates in its fresh table
  PinBuf<int> stats_h;                 // [0..15] read-back, [16..31] the neutral words
  PinBuf<unsigned long long> nvox_h;
  DevBuf<unsigned int> xcounts;        // export: per-block counts / offsets, their sum, then the scan's total (nb + 2 words)
  DevBuf<uint32_t> xslot, xslot2, xhi; // export: compacted slots (and in low-word order), high key words
  DevBuf<float> xout;                  // host export: [x | y | z | intensity] ...
  DevBuf<int32_t> xcnt;                // ... and counts
  DevBuf<int32_t> xijk;                // moments export: 3 ints per voxel ...
  DevBuf<double> xmom;                 // ... and its 9 sums
  DevBuf<int> tsel;                    // target from moments: what the selection pass reduces (TS_* words, ndt_map.hip)
  PinBuf<int> tsel_h;                  // [0..15] read-back, [16..31] the neutral words
  DevBuf<unsigned int> cmarks;         // carve (ndt_map_carve.hip): one call's mark word per slot, `capacity` of them
  DevBuf<unsigned long long> cstat;    // ... and its counters
  PinBuf<unsigned long long> cstat_h;
  // Components (ndt_map_components.hip): the union-find's parent word and the label per slot, `capacity` of each, the
  // component table on the device and on the host, the survivor flag per component of a removal.  The labelling is
  // cached: it stands while the map's `change`, the connectivity and min_count are those it was made under.
  DevBuf<uint32_t> ccparent;
  DevBuf<int32_t> cclabel;
  DevBuf<ndt_map_component> cccomps;
  DevBuf<int32_t> ccsurvive;
  std::vector<ndt_map_component> cccomps_h;
  ndt_map_components_info ccinfo{};
  bool cc_valid = false;
  uint64_t cc_change = 0;
  int cc_connectivity = 0, cc_min_count = 0;
  void release() {
    map_free_table(tab);
    moments = false;
    pkey.release(); px.release(); py.release(); pz.release(); ux.release(); uy.release(); uz.release(); ui.release();
    stats.release(); nvox.release(); stats_h.release(); nvox_h.release(); xcounts.release();
    xslot.release(); xslot2.release(); xhi.release(); xout.release(); xcnt.release(); xijk.release(); xmom.release();
    tsel.release(); tsel_h.release(); cmarks.release(); cstat.release(); cstat_h.release(); lchild.release();
    ccparent.release(); cclabel.release(); cccomps.release(); ccsurvive.release();
    cccomps_h.clear(); cccomps_h.shrink_to_fit();
    cc_valid = false;
  }
};

}  // namespace engine
}  // namespace ndt

using namespace ndt;
using namespace ndt::engine;

struct ndt_handle {
  ndt_params prm;
  int device = -1;
  KeepWarm keepwarm;                   // optional idle-time heartbeat (ndt_set_keepwarm), off by default
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;       // pre-launched evaluation kernels alternate between `stream` and this one
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  std::string err;

  // target
  // What is published and what became of its cloud: changed only by target_retire / target_publish / target_drop
  // (ndt_handoff.hip) and, for the cloud, by the producers' claim_cloud in front of their first write to tx/ty/tz.
  TargetState tgt;
  DevBuf<float> tx, ty, tz;          // the engine's own cloud: the first tgt.cloud_n() points are what the published grid was
                                     // built from (host targets, keyframes, map centroids); freed by a retire that keeps none
  FitIndex fit;                      // point-level nearest-neighbour index of getFitnessScore (ndt_fitness.hip)
  GridGeom geom{};
  int max_b[3] = {0, 0, 0};
  SortScratch sort;                  // the build's pair sort; the downsample, the voxel map and ndt_debug_sort_pairs reuse it
  PinBuf<BuildGeom> plan_h;          // host-written sort plans on their way to the device (sort_put_plan)
  unsigned plan_next = 0;            // ... and the next free slot of them
  DevBuf<int> nleaf;                 // [0] slots, [1] valid
  DevBuf<int> leaf_start, leaf_cnt, run_counts, run_offsets, fin_counts;
  std::unique_ptr<RepackPool> pool;   // repack workers of the host hand-off, created on first use
  DevBuf<uint32_t> sort_tags;         // tagged tile counts of the fused sort passes
  uint32_t sort_seq = 0;              // ... and their launch tag counter
  DevBuf<uint32_t> run_tags;          // tagged block leaf counts of the fused run search
  uint32_t run_seq = 0;
  long long n_fused_sort_fallbacks = 0;
  DevBuf<uint32_t> bucket_tab;        // two-launch build: where a tile holds a bucket's points, [bucket][tile] = {count : 16 | first : 16}
  DevBuf<int> bnd;                    // its 8 bounds words {min xyz, max xyz, #finite, largest bucket}; neutral between builds
  long long n_bucket_builds = 0, n_bucket_fallbacks = 0;
  long long n_chunked_pass_builds = 0, n_chunked_pass_launches = 0;   // host hand-offs whose partition ran under the transfer
  int bucket_skip = 0, bucket_backoff = 0;  // builds to go before the two-launch build is tried again after a decline
  const float* vx = nullptr;          // the source as evaluated: the engine's own copy (sx/sy/sz) or,
  const float* vy = nullptr;          // after ndt_set_source_device_view, the caller's arrays
  const float* vz = nullptr;
  unsigned int build_seq = 0;         // tag of the build whose completion the host polls for
  int n_cus = 0;                      // compute units of the device (a fused sort pass needs one per tile)
  DevBuf<double> leaf_sums;
  DevBuf<int> brows;                 // per-block bounds rows
  DevBuf<unsigned int> tickets;      // [0] bounds, [1] run-count, [2] finalize kernel, [4..5] the two-launch build's 64-bit tail word; zero between launches
  DevBuf<BuildGeom> gd;              // geometry + sort plan of the build, derived on the device
  PinBuf<BuildGeom> gdh;             // ... and its host-visible copy
  DevBuf<float> xyz4;                // packed float4 copy of the target for the gather
  IndexGrid cell2leaf;
  DevBuf<VoxelRecord> rec;
  // the same table as 48-byte PackedRecords (ndt_set_record_format): written behind every build while the packed
  // format is selected, or on demand when it is selected afterwards
  DevBuf<PackedRecord> prec;
  bool prec_valid = false;
  int record_format = NDT_RECORDS_F64;
  DevBuf<float> cent;                // 4 floats per leaf slot: f32 centroid (what the radius search tests) + chain link
  DevBuf<LeafStats> stats;
  double ms_build = 0;

  // source
  DevBuf<float> sx, sy, sz;
  size_t n_src = 0;
  ScanContextBufs sc;                // Scan Context: parameters, sector table, descriptor bank (ndt_scan_context.hip)
  D2dBufs d2d;                       // the distribution source of ndt_*_d2d and the target's leaves for it (ndt_d2d.hip)
  CtBufs ct;                         // the source's times and the scratch of ndt_*_ct (ndt_ct.hip)
  GicpBufs gicp;                     // GICP's parameters, neighbour lists, covariances and frozen pairs (ndt_gicp.hip)
  VgicpBufs vgicp;                   // voxelised GICP's table of per-leaf aggregates (ndt_vgicp.hip)
  EvalRowBufs evrows;                // the block rows and sums of a D2D, CT or GICP evaluation (ndt_eval_rows.hip)
  // the same points in block order of the target grid (see sort_source_by_blocks); valid until
  // the source or the target changes
  DevBuf<float> ox, oy, oz;
  SortScratch ssort;                 // the source ordering's own pair sort ...
  DevBuf<BuildGeom> splan;           // ... and its plan, written by k_source_keys
  bool src_sorted = false;
  int64_t n_src_global = -1;

  // staging
  // Host hand-off (ndt_set_target / ndt_set_source and their SoA forms): two lanes, each with its own pinned staging
  // buffer and stream, so that the target's transfer and build run while the source is repacked.
  struct UploadLane {
    PinBuf<float> stage;             // pinned, device-mapped staging: the cloud chunk by chunk as [x | y | z]
    hipEvent_t done = nullptr;       // the last pull kernel out of `stage` has finished
    hipEvent_t t0 = nullptr, t1 = nullptr;  // kernel timing: before the first copy / behind the last
    bool busy = false;               // `done` has been recorded and not yet waited for
    bool timed = false;              // t0 / t1 were recorded for the hand-off in flight
    ndt_handoff_lane_timing tm{};    // breakdown of the lane's last hand-off
  };
  UploadLane lane_t, lane_s;
  hipStream_t ustream = nullptr;     // the source lane's stream (the target lane shares `stream` with the build)
  hipStream_t pstream = nullptr;     // partition launches of a host target's build, beside the pull kernels on `stream` (created on first use)
  std::vector<hipEvent_t> pass_ev;   // ... one event per chunk in flight + the join
  bool src_upload_pending = false;   // the engine's streams have not yet been ordered behind the source hand-off
  int handoff_mode = NDT_HANDOFF_ASYNC;
  // The voxel-grid build of an asynchronous hand-off: enqueued by ndt_set_target, its verdict collected by the first
  // call that needs the grid (settle()).
  struct BuildRun {
    const float* x = nullptr;
    const float* y = nullptr;
    const float* z = nullptr;
    size_t n = 0;
    ndt_tuning tn{};             // build_begin's snapshot: every size and launch shape of this build, all attempts, follows it
    int dirty_slots = 0;
    size_t clean_cap = 0;
    bool fused = false, fused_sort = false, bucketed_ok = false;
    int min_pts = 0, max_leaves = 0;
    float leaf = 0, inv_leaf = 0;
    bool build_events = false, poll_done = false;
    std::chrono::steady_clock::time_point t0;
    // the attempt in flight
    int attempt = 0;
    bool optimistic = false, bucketed = false;
    int done_tag = 0;
    // the asynchronous host hand-off runs the two-launch build's partition under the transfer, chunk by chunk
    bool pass_chunked = false;   // attempt 0 finds its partition enqueued already (every tile)
    int pass_tiles = 0;          // tiles enqueued so far
  };
  BuildRun brun;
  bool build_pending = false;
  int deferred_rc = 0;               // status of a deferred build that failed, until a call that needs the grid (or ndt_wait) has reported it
  std::string deferred_msg;
  double ms_settle_wait = 0;         // time the collecting call waited for the pending build's verdict
  PinBuf<double> result;             // evaluation results (K * EV_WORDS)
  PinBuf<int> small;                 // bounds / counters read-back
  PinBuf<unsigned long long> flag;   // 32 result slots {seq, value} the single-pose kernel writes for the host
  DevBuf<double> partials, dres;
  CompactBufs compact;               // scratch of the filter's, the deskew's and the unprojection's compaction
  KnotTable knots;                   // the trajectory of the deskew / unprojection call in flight
  PointScoreBufs ps;                 // scratch of ndt_score_points / ndt_filter_source (ndt_point_scores.hip)
  DeskewBufs dsk;                    // scratch of ndt_deskew* / ndt_keyframe_put_deskewed (ndt_deskew.hip)
  ScanModelBufs scan;                // the scan model and the scratch of ndt_unproject* / ndt_keyframe_put_from_ranges (ndt_unproject.hip)
  PacketBufs pkt;                    // the packet format, the frame in progress and the scratch of the packet calls (ndt_packets.hip)
  DevBuf<unsigned int> counters;     // per-pose tickets of the in-kernel final reduction
  size_t counters_zeroed = 0;
  DevBuf<PoseConsts> dposes;
  PinBuf<PoseConsts> hposes;
  PoseConsts* bposes = nullptr;      // pose batch in BAR-mapped fine-grained device memory (host writes it directly)
  size_t bposes_cap = 0;
  size_t flag_slots = 0;             // poses the pinned result slots `flag` can hold

  // device-resident keyframe archive (pointsArchive of the drivers, ref: run/pipeline.cpp:784)
  struct Keyframe {
    DevBuf<float> x, y, z;
    size_t n = 0;
  };
  std::unordered_map<int64_t, Keyframe> keyframes;
  // buffers of erased keyframes, reused by the next ndt_keyframe_put (a sliding window erases one keyframe and archives
  // one per scan: hipMalloc / hipFree of three arrays each cost more than the upload they frame); at most 4 are kept
  std::vector<Keyframe> keyframe_pool;

  VoxelMap* map = nullptr;            // ndt_map_reset .. ndt_map_clear (ndt_map.hip); survives target builds and ndt_set_params
  VoxelMap* map_level[NDT_MAP_MAX_LEVEL] = {};   // [L - 1]: the map at leaf * 2^L, derived from the moments on demand and cached
                                                 // until the map changes (ndt_map_levels.hip); freed with the map

  // multi-grid target [RECALLED] (tier4 MultiGridNormalDistributionsTransform): the valid leaves of
  // every separately voxelised cloud, on the host (adding a map tile is not a per-scan operation);
  // ndt_multigrid_create_kdtree assembles their union into the device table
  struct MultiGridEntry {
    std::vector<VoxelRecord> rec;
    std::vector<LeafStats> stats;
    std::vector<int> ijk;  // absolute lattice index of every leaf, 3 ints
    size_t n_points = 0;
    float resolution = 0.0f;
    int min_points = 0, cov_mode = 0;
    double eig_ratio = 0.0;
  };
  std::map<int64_t, MultiGridEntry> mgrids;
  std::vector<LeafStats> multi_stats; // the union's leaves in table order, for export (tgt.is_union(): the device table is
                                      // the union -- neighbourhood: radius search, chained cells)

  // pre-launched evaluation (ndt_prelaunch): mailbox in BAR-mapped fine-grained device memory
  PoseMailbox* mbox = nullptr;
  bool mbox_tried = false;
  bool mbox_tagged = true;            // the pose is published as tagged 8-byte granules
  bool mbox_preload = false;          // the waiting kernel fetches its points before the pose arrives (measured: no gain)
  bool prelaunch_armed = false;       // inside ndt_align
  struct Waiting {                    // the kernel enqueued for the NEXT evaluation: set together, claimed together (evaluate())
    unsigned long long seq = 0;       // sequence number of the kernel that is waiting, 0 = none
    unsigned long long round = 0;     // ... and the cross-rank round it will exchange under (NDT_REDUCE_P2P)
    int on2 = 0;                      // ... and the stream it is on (0: stream, 1: stream2)
    int buf = 0;                      // ... and the result buffer (0 / 1) it will write
    bool need_h = false;              // ... and whether it computes the Hessian (an evaluation that differs sends it away)
    DerivLaunchPlan plan{};           // the shape of the waiting kernel's launch (evaluation log)
  } pre;
  int cur_on2 = 0;                    // stream of the evaluation in flight
  bool two_streams = true;            // NDT_PRELAUNCH_STREAMS != 1
  // NDT_PRELAUNCH_AUTO decides between the two-stream and the one-stream placement of the waiting kernel BY MEASUREMENT:
  // a waiting kernel on the other stream holds its compute units for the whole evaluation of its predecessor -- harmless
  // on a device the engine has to itself, ruinous when another engine's kernels need those units (two ranks on one
  // device: 0.97 against 0.59 ms per step, HISTORY section 5).  The handle keeps the best recent wall time per
  // launched evaluation in the placement in use and runs the 6th, the 14th and then every 32nd align in the other one as a probe; a probe that is
  // 15 % faster switches the handle over (and the probing goes on from there, so it can switch back).
  bool auto_one_stream = false;       // the placement AUTO currently uses
  bool probing = false;               // this align runs in the other placement
  bool streams_this_align = true;     // two-stream placement in effect for the align in flight
  double us_eval_mean[2] = {0.0, 0.0};  // best recent wall time per launched evaluation: [0] two streams, [1] one stream; 0 = no sample yet
  int64_t n_auto_aligns = 0, n_auto_switches = 0;
  DevBuf<unsigned int> arrive_ctr;    // [2] blocks of a pre-launched launch that have started (per result buffer)
  PinBuf<unsigned long long> arrived; // [2] sequence number of the launch whose blocks are all resident
  int prelaunch_strikes = 0;          // consecutive aligns in which a waiting kernel gave up
  bool prelaunch_suspended = false;   // three such aligns in a row (a chronically starved host): no more pre-launching
                                      // on this handle until ndt_set_params is called -- the caller's ndt_params
                                      // are never rewritten
  int flag_toggle = 0;                // result buffer of the latest single-pose launch
  int64_t n_prelaunch_used = 0, n_prelaunch_quit = 0, n_prelaunch_timeouts = 0;
  int64_t n_lost_row_retries = 0;      // evaluations repeated through the ticketed final sum after a row was lost
  // The first evaluation of an align that follows a DEFERRED build is enqueued behind that build, before its verdict is
  // known (evaluate()): spec_first is set by ndt_align for its first evaluate() call.
  bool spec_first = false;
  bool spec_enabled = true;            // (ndt_debug_set_speculation: in-process A/B)
  bool spec_build_failed = false;      // the deferred build's failure surfaced inside that first evaluation
  int64_t n_spec_used = 0, n_spec_discarded = 0;
  int64_t n_p2p_host_finishes = 0;     // peer-write evaluations whose exchange the host finished (a peer was late)
  int64_t n_prelaunch_overlapped = 0; // pre-launches that went to the other stream (resident before their predecessor ended)

  // evaluation log (ndt_debug_eval_log): off (cap 0) by default; entries beyond cap are counted, not kept
  int eval_log_cap = 0;
  int64_t eval_log_total = 0, eval_log_launches = 0;
  std::vector<EvalLogEntry> eval_log;

  bool have_reg = false;
  float reg_pose[16];
  IterHistory history;                // per-iteration transforms / scores of the last ndt_align (ndt_get_iteration_history)

  Reducer red;

  bool timing = false;
  ndt_timing tm{};
};


#define HIP_TRY(h, expr)                                                                  \
  do {                                                                                    \
    hipError_t e__ = (expr);                                                              \
    if (e__ != hipSuccess)                                                                \
      return fail(h, (e__ == hipErrorOutOfMemory) ? NDT_ERR_ALLOC : NDT_ERR_HIP,          \
                  std::string(#expr) + ": " + hipGetErrorString(e__));                    \
  } while (0)

namespace ndt {
namespace engine {

int fail(ndt_handle* h, int code, const std::string& msg);
// a selection of n points that the caller's output does not hold
inline int over_capacity(ndt_handle* h, size_t n) {
  return fail(h, NDT_ERR_INVALID_ARG, "output capacity too small: " + std::to_string(n) + " points selected");
}
int bind_device(ndt_handle* h);
bool params_valid(const ndt_params* p, std::string* why);
int lane_wait(ndt_handle* h, ndt_handle::UploadLane& lane);
int upload_soa(ndt_handle* h, ndt_handle::UploadLane& lane, hipStream_t stream, const float* xyz, const float* x,
               const float* y, const float* z, size_t n, size_t stride, DevBuf<float>& dx, DevBuf<float>& dy,
               DevBuf<float>& dz, bool sync, const std::function<void(size_t /* points on the device so far */, bool /* last chunk */)>* after_chunk = nullptr);
int pack_records(ndt_handle* h, bool wait);
int records_for_eval(ndt_handle* h, EvalConsts* ec, const VoxelRecord** rec);
int neutral_bounds(ndt_handle* h);
// The target's three transitions on a handle (ndt_handoff.hip; the state itself: ndt_target_state.h).
// target_retire: the published target makes way for the one being produced -- the cached source order and packed records
// go with it, nothing is pending or deferred any more, and tx/ty/tz are freed unless their first kept_cloud_n points are
// what the new grid is built from.  Returns the index grid's reuse pair.
IndexReuse target_retire(ndt_handle* h, size_t kept_cloud_n);
// target_publish: the produced grid becomes the target (n_slots == n_valid == the leaves of a UNION); behind a SINGLE the
// packed records are written while that format is selected.
int target_publish(ndt_handle* h, TargetKind kind, const GridGeom& geom, const int max_b[3], size_t n_points, int n_slots,
                   int n_valid, double ms);
void target_drop(ndt_handle* h);
// the geometry of a grid of edge `leaf` over the lattice box mn .. mx (inclusive; the caller has checked: fewer than 2^31 cells)
template <typename I>
GridGeom grid_geom_from_box(float leaf, const I mn[3], const I mx[3]) {
  GridGeom g{};
  g.leaf = leaf;
  g.inv_leaf = 1.0f / leaf;
  for (int a = 0; a < 3; ++a) {
    g.min_b[a] = (int)mn[a];
    g.div_b[a] = (int)(mx[a] - mn[a] + 1);
    g.lo[a] = (float)g.min_b[a] * g.leaf;
    g.hi[a] = (float)(mx[a] + 1) * g.leaf;
  }
  g.mul1 = g.div_b[0];
  g.mul2 = g.div_b[0] * g.div_b[1];
  g.ncells = g.mul2 * g.div_b[2];
  return g;
}
// ---- the keyed sort on a handle (ndt_sort.hip) ----
// A plan for `bits`-bit keys (1 .. 32) and `ncells`, status BG_OK, copied to the device plan `d_plan` on the engine's
// stream; *passes: its digit passes.  The copy's source must live until the copy has run, so it is one of SORT_PLAN_SLOTS
// pinned slots of the handle (h->plan_h) taken in turn, and the writer waits for the stream whenever it starts the
// round again: no slot is rewritten while a copy out of it can still be pending, however many plans a call enqueues.
constexpr unsigned SORT_PLAN_SLOTS = 8;
int sort_put_plan(ndt_handle* h, BuildGeom* d_plan, int bits, int ncells, int* passes);
// The one sort call: the n pairs (sc.keys, identity) stably sorted on the key bits of the plan in *d_plan (device memory;
// nothing runs unless its status is BG_OK) in `passes` digit passes, enqueued on s.  The passes need the first digit's tile
// histograms in sc.tmp: SORT_FIRST_COUNTED says the kernel that wrote the keys counted them on its way (launch_cell_keys,
// k_source_keys), SORT_COUNT_FIRST makes this call launch the count.  *out: where the sorted keys and values are.
enum SortFirstDigit { SORT_COUNT_FIRST = 0, SORT_FIRST_COUNTED = 1 };
hipError_t sort_keyed(SortScratch& sc, size_t n, const BuildGeom* d_plan, int passes, SortFirstDigit first, hipStream_t s,
                      SortedPairs* out);
// What a sort on the handle's scratch and the run search behind it work in, for n pairs and at most max_runs runs: the
// build's BuildGeom (device + pinned), the tickets (zero), the plan slots, h->sort, the leaf counters and lists, the run
// search's block counts.  The build passes its max_leaves, everyone else n + 1.
int group_scratch(ndt_handle* h, size_t n, size_t max_runs);
// launch_find_runs on the handle's buffers (after group_scratch): runs of equal keys with >= min_pts entries -> h->nleaf,
// h->leaf_start, h->leaf_cnt; fused: count and emit in one launch (the build with ndt_tuning::fused_sort on)
hipError_t find_runs(ndt_handle* h, const uint32_t* keys_sorted, size_t n, int min_pts, bool fused);
int build_begin(ndt_handle* h, const float* x, const float* y, const float* z, size_t n, ndt_handle::BuildRun& br);
int build_enqueue(ndt_handle* h, ndt_handle::BuildRun& br);
int build_collect(ndt_handle* h, ndt_handle::BuildRun& br);
int build_complete(ndt_handle* h, ndt_handle::BuildRun& br);
int build_grid(ndt_handle* h, const float* x, const float* y, const float* z, size_t n, bool defer = false);
int settle_build(ndt_handle* h);
int settle_source(ndt_handle* h);
int source_behind_target_transfer(ndt_handle* h, bool async);
int report_deferred(ndt_handle* h);
int settle(ndt_handle* h);
void settle_discard_keep_grid(ndt_handle* h);
void settle_discard(ndt_handle* h);
// ndt_keyframes.hip: the archive entry `id` for a scan of n points -- a new entry takes pooled buffers that are large
// enough, a replaced one that is the viewed source unsets the source; the caller fills x / y / z and sets n
ndt_handle::Keyframe& keyframe_claim(ndt_handle* h, int64_t id, size_t n);
// ndt_point_scores.hip: a compaction's host side around its three launches.  compact_scratch makes h->compact hold nb
// blocks; compact_total, behind the launches, reports a launch error, fetches the scan's total into *n_out (awaited) and
// refuses one above cap
int compact_scratch(ndt_handle* h, int nb);
int compact_total(ndt_handle* h, int nb, size_t cap, size_t* n_out);
// ndt_deskew.hip: rows[0 .. n_knots) -> h->knots through its pinned staging, enqueued on the engine's stream (n_knots = 0:
// the table is only allocated)
int knots_upload(ndt_handle* h, const traj::KnotRow* rows, int n_knots);
// ---- the host-cloud boundary's engine half (ndt_handoff.hip; the pure host half and the layout rule: ndt_host_cloud.h) ----
// upload_column: the float byte_offset into every point of a strided host cloud -> dst[0 .. n), gathered into pageable
// memory and copied with a blocking copy (the intensity column of the host forms that take one)
int upload_column(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, size_t byte_offset, DevBuf<float>& dst);
// the tight arrays of a device result that go down beside its cloud, m elements each: one of floats (the points' times)
// and one of int32 (the points' indices; ndt_map_export's per-voxel counts).  A null host pointer: not wanted.
struct SideColumns {
  const float* d_f32 = nullptr;
  float* f32_out = nullptr;
  const int32_t* d_i32 = nullptr;
  int32_t* i32_out = nullptr;
};
// download_strided: the first m points of a device result -- columns [x | y | z | intensity] col_stride floats apart at
// d_cols -- to a strided host cloud (layout_valid) through the host staging `back` (m floats per column; null: a vector
// of this call), the side columns directly; awaited.  m > cap is refused with nothing written, m = 0 copies nothing.
int download_strided(ndt_handle* h, const float* d_cols, size_t col_stride, size_t m, size_t cap, float* out, size_t stride_bytes,
                     long intensity_offset_bytes, float* back = nullptr, const SideColumns& side = SideColumns());
// ndt_unproject.hip, for the packet forms (ndt_packets.hip): what every unprojection checks before anything is written
// (the model, the gate, the trajectory into rows), and the launches on device arrays whose arguments have been checked
int unproject_check(ndt_handle* h, const ndt_range_gate* gate, const double* knot_t, const double* knot_poses16, int n_knots,
                    const double* ref16, traj::KnotRow* rows);
int unproject_device(ndt_handle* h, const uint32_t* d_range, const uint8_t* d_refl, const float* d_col_t, const ndt_range_gate* gate,
                     const traj::KnotRow* rows, int n_knots, const ndt_scan_filter* filter, float* ox, float* oy, float* oz, float* oi,
                     float* ot, int32_t* o_index, size_t cap, size_t* n_out);
void map_release(ndt_handle* h);   // ndt_map.hip: frees the voxel map, if any (ndt_destroy)
// ndt_map.hip's host side as ndt_map_state.hip uses it (the kernels stay where they are)
constexpr int64_t MAP_MAX_CAPACITY = 1ll << 30;   // slots are 32-bit sort keys with one sentinel above them
int no_map(ndt_handle* h);
int64_t map_pow2_at_least(int64_t v);
int map_box_floor(float v, float inv_leaf);
bool pose_finite(const double p[16]);
bool finite3(const float v[3]);
int map_alloc_table(ndt_handle* h, int64_t cap, bool with_moments, MapTable* t);
// The map's table is replaced by a fresh one of new_cap slots that `launch` fills from the old one (the caller's launches
// on the engine's stream, awaited here; a launch that returns an error has reported it).  kept == -1: growth, every voxel
// moves.  kept >= 0: a selective move that keeps `kept` voxels -- tsel is reset in front of the launch and read back
// behind it, the device's voxel counter, n_voxels and (kept > 0) the ijk box follow.  kept == MAP_KEPT_COUNTED: the launch
// counts the voxels it creates in nvox[1] (zeroed in front of it); the device's voxel counter and n_voxels follow, the ijk
// box is the caller's.  On any error the map is as it was and `what` heads the text.
constexpr int64_t MAP_KEPT_COUNTED = -2;
int map_replace_table(ndt_handle* h, VoxelMap& m, int64_t new_cap, const char* what,
                      const std::function<int(const MapTable&)>& launch, int64_t kept);
// what fills the fresh table in place of growth's move (map_grow_table)
struct MapRefill {
  const char* what;
  std::function<int(const MapTable&)> launch;
};
int map_grow_table(ndt_handle* h, VoxelMap& m, int64_t new_cap, const MapRefill* refill = nullptr);
// (the VoxelMap a function takes is the map, *h->map, or one of its levels, h->map_level[]: ndt_map_levels.hip)
int map_init_buffers(ndt_handle* h, VoxelMap& m);   // the small device / pinned words every VoxelMap works with
int map_refresh_voxel_count(ndt_handle* h, VoxelMap& m);
int map_group_batch(ndt_handle* h, VoxelMap& m, size_t n, const MapTable& t, unsigned long long* d_nvox,
                    const uint32_t** keys_sorted, const uint32_t** vals_sorted);
int map_export_count(ndt_handle* h, VoxelMap& m, const MapSel& sel, bool box, size_t* total);
int map_export_order(ndt_handle* h, VoxelMap& m, const MapSel& sel, bool box_sel, size_t total, const int mn[3], const int mx[3],
                     const uint32_t** order_out, const uint32_t** slots_out);
int no_moments(ndt_handle* h);
// ndt_set_target_from_map_moments behind its argument checks, for the map or a level of it
int target_from_moments(ndt_handle* h, VoxelMap& m, const float* box_min, const float* box_max);
void map_levels_release(ndt_handle* h);   // ndt_map_levels.hip: frees the cached levels (the stream is idle)
// ndt_map_state.hip's host side as ndt_map_repose.hip uses it: the state export into device arrays (awaited), the checks
// of an import once the map is known, the import behind its key pass (one host wait, refusals, growth, counters, merge;
// awaited) and the merge itself into a given table (enqueued)
int map_export_state(ndt_handle* h, VoxelMap& m, const float* box_min, const float* box_max, int32_t* d_ijk, int32_t* d_count,
                     float* d_sums, double* d_mom, size_t cap, size_t* total_out);
// both public export forms behind the handle checks (box, moments, outputs as ndt_map_export_state[_device] takes them)
int map_export_state_public(ndt_handle* h, VoxelMap& m, bool device_out, const float* box_min, const float* box_max, int32_t* ijk,
                            int32_t* count, float* sums4, double* moments9, size_t cap, size_t* n_out);
int map_import_checks(ndt_handle* h, float leaf, const double* moments9, size_t n, bool* go);
int map_import_tail(ndt_handle* h, const int32_t* d_count, const float* d_sums, const double* d_mom, size_t n);
int map_merge_records(ndt_handle* h, const MapTable& t, unsigned long long* d_nvox, const int32_t* d_count, const float* d_sums,
                      const double* d_mom, size_t n);
// ndt_fitness.hip: the point-level index `f` (re)built over the SoA cloud x / y / z (device memory, n points), enqueued
// on the engine's stream behind one host wait; `what` heads the error texts.  fit_build: the handle's `fit` over the
// engine's copy of the target, lazily (the target is settled).
int fit_build_cloud(ndt_handle* h, FitIndex& f, const float* x, const float* y, const float* z, size_t n, const char* what);
int fit_build(ndt_handle* h);
// ndt_gicp.hip's host side as ndt_vgicp.hip uses it: one rank and the streams settled; what a target / a source must be;
// the target's and the source's neighbour lists and covariances (h->gicp.tgt / h->gicp.src), derived if they are not fresh
int gicp_settle(ndt_handle* h);
int gicp_target_state(ndt_handle* h);
int gicp_target_ready(ndt_handle* h);
int gicp_source_ready(ndt_handle* h);
// ndt_eval_rows.hip: what the lane-per-item evaluations (D2D, CT, GICP, VGICP) share behind their kernels.  `what` is "D2D", "CT"
// or "GICP" and heads the error texts.
// k_eval_rows_sum on rows of K poses x nb blocks x EV_WORDS -> out (K x EV_WORDS), enqueued on s
void launch_eval_rows_sum(const double* rows, int nb, int K, double* out, hipStream_t s);
// what such an evaluation can work with: one rank, DIRECT1 / DIRECT7, a single grid -- and a target to evaluate against
int lane_eval_supported(ndt_handle* h, const char* what);
// K poses -> K x EV_WORDS raw sums in `out`: launch(k, rows) enqueues pose k's kernel (nb blocks, one row each) on the
// engine's stream; then the fixed-order sum, the copy and the wait.  A score that is not finite fails.
int lane_eval_rows(ndt_handle* h, const char* what, int nb, int K, const std::function<void(int, double*)>& launch, double* out);
// raw sums -> what ndt_eval_derivatives hands out: ridge / regularisation / guards (finish_eval), repacked in place
void finish_words(ndt_handle* h, const double pose6[6], bool need_h, double* w);
// newton_align over an evaluation of n_items items: raw(pose6, need_h, words) fills one pose's raw sums
using LaneEvalFn = std::function<int(const double*, bool, double*)>;
// (prm: the parameters of the loop and of finish_eval; null: the handle's)
int lane_align(ndt_handle* h, int64_t n_items, const float guess[16], const LaneEvalFn& raw, ndt_result* out,
               const ndt_params* prm = nullptr);
void fill_pose_consts(const double p[6], const float T[16], PoseConsts* pc);
unsigned long long process_item_salt();
EvalConsts make_eval_consts(const ndt_handle* h, bool need_h);
int ensure_counters(ndt_handle* h, size_t k);
int ready_for_eval(ndt_handle* h);
int ensure_flag_slots(ndt_handle* h, size_t K);
int maybe_sort_source(ndt_handle* h, const float T[16]);
bool source_sort_wanted(const ndt_handle* h, int n_valid);
bool first_eval_behind_build(const ndt_tuning& tn, const ndt_handle* h);
int ensure_partials(ndt_handle* h, size_t words);
bool slots_complete(const volatile unsigned long long* slots, unsigned long long seq);
int wait_slots(ndt_handle* h, unsigned long long seq, int K = 1, int first = 0);
bool ensure_mailbox(ndt_handle* h);
void publish_pose(ndt_handle* h, unsigned long long seq, const PoseConsts& pc);
void quit_prelaunched(ndt_handle* h);
int evaluate(ndt_handle* h, const double p[6], const float T[16], bool need_h, Eval* out, bool score_only = false,
             bool safe_retry = false);
// appends K entries (one launch) to the evaluation log; words: K x EV_WORDS, T: K x 16, poses6: K x 6
void log_evals(ndt_handle* h, const DerivLaunchPlan& plan, const double* poses6, const float* T, const double* words, int K,
               bool need_h, bool score_only, bool prelaunched);

}  // namespace engine
}  // namespace ndt
