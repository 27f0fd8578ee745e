/*
 * ndt_hip.h -- C-ABI of the MI355X-native NDT scan-matching engine.
 *
 * This is the drop-in boundary for the registration path of khalisfadil/slam-sam:
 * the `pcl::Registration<PointXYZI,PointXYZI>::Ptr registration` member of
 * RegisterCallback (ref: include/registercallback.hpp:35) which the drivers fill
 * with a `pclomp::NormalDistributionsTransform` (ref: run/pipeline.cpp:464-481)
 * and drive with setInputTarget / setInputSource / align / getFinalTransformation
 * / getResult (ref: run/pipeline.cpp:557-568, run/pipeline_ligo_tc.cpp:529-538).
 * The C++ adapter include/ndt_hip/ndt_hip.hpp maps those method names onto the
 * functions below; INTEGRATION.md shows the reference-side binding.
 *
 * Conventions (all citations relative to the reference tree):
 *  - plain C: opaque handle, POD structs, caller-allocated outputs; every call
 *    returns an ndt_status (0 = ok, < 0 = error) and never throws.  The engine
 *    needs a gfx950 device: without one every compute entry point fails with
 *    NDT_ERR_NO_DEVICE -- there is no CPU fallback.
 *  - matrices are 4x4 float, COLUMN-major (Eigen::Matrix4f layout), source ->
 *    target frame (ref: run/pipeline.cpp:561,566).
 *  - the 6-vector pose is [x, y, z, roll, pitch, yaw] with R = Rx*Ry*Rz
 *    (ref: extern/svn_ndt/include/svn_ndt_impl.hpp:256-260,272-279).
 *  - score / gradient / Hessian are those of the POSITIVE score that NDT
 *    maximises, so the Hessian is negative definite near the optimum and callers
 *    form cov = -(H + 1e-6 I)^-1 (ref: run/pipeline.cpp:594-596).  Hessians are
 *    6x6 double, row-major (symmetric).
 *  - a handle is NOT thread-safe; distinct handles are independent (the
 *    reference uses one engine per thread, ref: run/pipeline.cpp:432,464).
 *  - the engine never keeps caller pointers after a call returns: a cloud handed
 *    over from host memory has been read completely when ndt_set_target /
 *    ndt_set_source return (the caller may free or overwrite it at once), even
 *    though its transfer and the target's voxel-grid build may still be running
 *    on the device (asynchronous hand-off, below).
 */
#ifndef NDT_HIP_H_
#define NDT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDT_HIP_ABI_VERSION 3

typedef enum ndt_status {
  NDT_OK = 0,
  NDT_ERR_INVALID_ARG = -1,
  NDT_ERR_NO_DEVICE = -2,   /* no usable gfx950 device / HIP runtime failure at init */
  NDT_ERR_HIP = -3,         /* a HIP call failed; see ndt_last_error() */
  NDT_ERR_NO_TARGET = -4,   /* align/eval before a target with >= 1 valid voxel */
  NDT_ERR_NO_SOURCE = -5,
  NDT_ERR_GRID_OVERFLOW = -6, /* dx*dy*dz > INT32_MAX (ref: voxel_grid_covariance_impl.hpp:108-125) */
  NDT_ERR_ALLOC = -7,
  NDT_ERR_COMM = -8,        /* RCCL / shared-memory reduction failure */
  NDT_ERR_UNSUPPORTED = -9,
  NDT_ERR_INTERNAL = -10    /* a bounded device loop ran out of its bound (ndt_map_components*): a defect, never a wait */
} ndt_status;

/* same order as pclomp::NeighborSearchMethod (ref: run/pipeline.cpp:471-480) */
typedef enum ndt_search_method {
  NDT_KDTREE = 0,   /* radius search (radius = resolution) over voxel centroids
                       (ref: voxel_grid_covariance_impl.hpp:505-554), done as a 27-cell scan */
  NDT_DIRECT26 = 1, /* [RECALLED] pclomp getNeighborhoodAtPoint: every valid voxel of the 3x3x3 block around the
                       point's cell, enumerated in integer index space.  The reference tree holds only the
                       enum value (run/pipeline.cpp:471-480) and a commented stub (svn_ndt_impl.hpp:581-583) */
  NDT_DIRECT7 = 2,
  NDT_DIRECT1 = 3
} ndt_search_method;

typedef enum ndt_hessian_mode {
  NDT_HESSIAN_FULL = 0,         /* Magnusson eq. 6.13 (pclomp; svn_ndt_impl.hpp:472-494) */
  NDT_HESSIAN_GAUSS_NEWTON = 1  /* J^T C^-1 J only (svn default, svn_ndt_impl.hpp:496-499) */
} ndt_hessian_mode;

typedef enum ndt_cov_mode {
  NDT_COV_SVN = 0,          /* ss/n - mu mu^T, * n/(n-1)  (voxel_grid_covariance_impl.hpp:287-291) */
  NDT_COV_PCL_RECALLED = 1  /* upstream PCL form, * (n-1)/n -- recalled, unverifiable offline */
} ndt_cov_mode;

typedef enum ndt_reduce_mode {
  NDT_REDUCE_NONE = 0, /* single GPU */
  NDT_REDUCE_RCCL = 1, /* ncclAllReduce of the 32-double partial over xGMI */
  NDT_REDUCE_SHM = 2,  /* pinned-host partials summed through POSIX shared memory */
  NDT_REDUCE_HOOK = 3, /* caller-supplied all-reduce callback */
  NDT_REDUCE_P2P = 4   /* one-shot peer-write all-gather over xGMI + local sum, INSIDE the derivative
                          kernel's final sum: no collective launch, no host hop, and the host-polled /
                          pre-launched fast path of a single GPU stays on */
} ndt_reduce_mode;

typedef enum ndt_wait_mode {
  NDT_WAIT_SPIN = 0,   /* the calling thread polls the result slots in pinned memory (lowest latency;
                          occupies one host core for the duration of ndt_align) */
  NDT_WAIT_BLOCK = 1   /* the calling thread sleeps in hipStreamSynchronize (+3..4 us per evaluation;
                          for hosts that cannot spare a core: the drivers run 6-7 threads + OpenMP) */
} ndt_wait_mode;

typedef enum ndt_source_order {
  NDT_SOURCE_ORDER_AUTO = 0, /* sort when the voxel table is larger than one L2 (records > 6 MB) and the
                                source has >= 32768 points */
  NDT_SOURCE_ORDER_KEEP = 1, /* evaluate the source in the order it was handed over */
  NDT_SOURCE_ORDER_SORT = 2  /* always: once per align, the source is stably sorted by the block of target
                                voxels its points fall into under the initial guess (a wavefront then touches
                                few distinct voxel records; only the f64 summation order changes) */
} ndt_source_order;

typedef enum ndt_prelaunch {
  NDT_PRELAUNCH_AUTO = 0, /* inside ndt_align (spin wait, no RCCL reducer): the kernel of the next evaluation is
                             enqueued while the current one runs and waits on the device for its pose, which the
                             host publishes through BAR-mapped device memory -- takes the launch + dispatch latency
                             (~4 us of ~7) out of every evaluation but the first.  Successive kernels alternate
                             between two streams of the engine, so that the next one takes compute units as the
                             blocks of the one in flight leave.  Used when the device exposes a large BAR; a kernel
                             that waited 20 ms gives up and the pose is evaluated through an ordinary launch.
                             The two-stream placement is right for a device the engine has to itself; AUTO checks that
                             by measurement (the 6th, the 14th and then every 32nd align run with the one-stream placement; one that is 15 %
                             faster per evaluation switches the handle over, and back the same way), so a second
                             engine or process on the same device is noticed without being told. */
  NDT_PRELAUNCH_OFF = 1,
  NDT_PRELAUNCH_ONE_STREAM = 2 /* as AUTO, but every kernel stays on the engine's one stream (the next starts when the
                             current one has ENDED).  For several engines / processes that share ONE device: a
                             waiting kernel holds its compute units, and with two streams it holds them for the
                             whole evaluation of its predecessor -- units the other engine's running kernel needs. */
} ndt_prelaunch;

/* Named parameter sets.  ndt_default_params() is the vendored-code hybrid the parity tests pin
 * (svn covariance, full Hessian, no ridge, More-Thuente); the presets restate the two engines. */
typedef enum ndt_preset {
  NDT_PRESET_DEFAULT = 0,
  NDT_PRESET_PCLOMP_RECALLED = 1, /* upstream pclomp as recalled: PCL covariance normalisation
                                     (n-1)/n, full Hessian, no ridge, More-Thuente line search, min 6 points */
  NDT_PRESET_SVN = 2              /* vendored svn_ndt: n/(n-1) covariance, Gauss-Newton Hessian, +1e-6 I */
} ndt_preset;

/* Parameter block; mirrors the pclomp / svn_ndt setters the drivers call and
 * RegisterCallback's JSON fields (ref: include/registercallback.hpp:37-54,
 * src/registercallback.cpp:24-91). */
typedef struct ndt_params {
  float resolution;              /* setResolution; voxel leaf size in metres */
  double step_size;              /* setStepSize; More-Thuente step_max */
  double trans_epsilon;          /* setTransformationEpsilon */
  int max_iterations;            /* setMaximumIterations */
  double outlier_ratio;          /* setOutlierRatio (0.55) */
  int search_method;             /* ndt_search_method */
  int min_points_per_voxel;      /* 6; clamped to >= 3 (voxel_grid_covariance.h:153,176-184) */
  double eig_inflation_ratio;    /* 0.01 (voxel_grid_covariance.h:154) */
  int hessian_mode;              /* ndt_hessian_mode */
  int cov_mode;                  /* ndt_cov_mode */
  int add_ridge;                 /* H += 1e-6 I after accumulation (svn_ndt_impl.hpp:650-653) */
  int use_line_search;           /* 1: More-Thuente; 0: fixed step min(|dp|, step_size) */
  float regularization_scale_factor; /* setRegularizationScaleFactor (run/pipeline_ligo_tc.cpp:293) */
  int num_threads;               /* setNumThreads; recorded only -- there is no CPU path */
  int device_id;                 /* HIP device ordinal; -1 = current device */
  int wait_mode;                 /* ndt_wait_mode */
  int source_order;              /* ndt_source_order */
  int prelaunch;                 /* ndt_prelaunch */
} ndt_params;

typedef struct ndt_handle ndt_handle;

/* pclomp::NdtResult + pcl::Registration outputs (ref: run/pipeline.cpp:566-568,594;
 * include/map.hpp:96-97 for the two timing/iteration statistics). */
typedef struct ndt_result {
  float final_transformation[16]; /* getFinalTransformation(), column-major */
  double final_pose[6];           /* [x,y,z,roll,pitch,yaw] */
  int converged;                  /* hasConverged() */
  int iterations;                 /* getFinalNumIteration() / NdtResult::iteration_num */
  int n_evaluations;              /* derivative evaluations incl. line-search trials */
  double hessian[36];             /* NdtResult::hessian, row-major */
  double score;
  double transform_probability;   /* score / #source points */
  double nearest_voxel_transformation_likelihood;
  int64_t n_pairs;                /* (point, voxel) pairs of the last evaluation */
  int64_t n_points_with_neighbors;
  double ms_total;                /* wall time of ndt_align */
  double ms_device;               /* sum of device-side evaluation time (HIP events) */
  int n_evaluations_reused;       /* line-search requests at the pose of the evaluation before them
                                     (a step clamped to its lower bound is re-tried up to 10 times):
                                     answered without a launch, bit-identical by construction */
} ndt_result;

/* Per-voxel statistics, the accessors extractNdtData() uses
 * (ref: include/pipeline.hpp:175-206; Leaf: voxel_grid_covariance.h:99-131). */
typedef struct ndt_leaf {
  int64_t index;     /* 1-D voxel index ijk0 + ijk1*div_x + ijk2*div_x*div_y */
  int32_t point_count;
  float center[3];   /* getLeafCenter(index) */
  double mean[3];
  double cov[9];     /* row-major */
  double icov[9];
  double evecs[9];   /* eigenvectors as columns, eigenvalues ascending */
  double evals[3];
} ndt_leaf;

typedef struct ndt_grid_info {
  int min_b[3], max_b[3], div_b[3];
  float leaf_size, inverse_leaf_size;
  int64_t n_leaves;        /* valid voxels */
  int64_t n_cells;         /* dx*dy*dz of the dense index grid */
  int64_t n_target_points;
  double ms_build;         /* time of the last target build: device time (HIP events) while kernel timing is enabled, wall time of the call otherwise */
} ndt_grid_info;

/* one derivative evaluation: [score, g(6), H upper-tri (21), nvtl_sum,
 * n_points_with_neighbors, n_pairs, pad] */
#define NDT_EVAL_WORDS 32

/* ---- lifecycle ---------------------------------------------------------- */
int ndt_abi_version(void);
void ndt_default_params(ndt_params* p);
/* overwrites the algorithm switches of *p (cov_mode, hessian_mode, add_ridge, use_line_search,
 * min_points_per_voxel) with a named set; everything else is left as it is */
int ndt_params_preset(ndt_params* p, int preset /* ndt_preset */);
int ndt_create(const ndt_params* p, ndt_handle** out);   /* new pclomp::NormalDistributionsTransform */
int ndt_destroy(ndt_handle* h);
int ndt_set_params(ndt_handle* h, const ndt_params* p);  /* a changed resolution rebuilds the grid */
int ndt_get_params(const ndt_handle* h, ndt_params* p);
const char* ndt_last_error(const ndt_handle* h);
/* human-readable device description; returns the number of visible devices or < 0 */
int ndt_backend_info(char* buf, size_t cap);

/* ---- clouds ------------------------------------------------------------- */
/* Hand-off of HOST clouds (the drivers hold host pcl::PointCloud<PointXYZI>, ref: run/pipeline.cpp:554-561).
 * NDT_HANDOFF_ASYNC (default): ndt_set_target / ndt_set_source (and their _soa forms) return as soon as the
 * caller's memory has been repacked into the engine's pinned staging; the PCIe copies, the SoA conversion and the
 * target's voxel-grid build run behind on the device, the target's under the source's repack, and the first call
 * that needs them (ndt_align, ndt_eval_derivatives, ndt_get_grid_info, ndt_export_leaves, ...) waits for them.
 * Consequence: a steady-state build that FAILS (no finite point, index overflow) is reported by that first call
 * (or by ndt_wait), with the same status code, not by ndt_set_target -- the reference's setInputTarget returns
 * void, its failures surface in align the same way (ref: svn_ndt_impl.hpp:682-702).  The first build of a handle,
 * the build that follows a failed one (both wait for the grid geometry inside the call), an empty cloud and
 * argument errors are still reported at once.
 * NDT_HANDOFF_SYNC: both calls block until the device has everything (rounds 1-3 behaviour; also NDT_HANDOFF=sync
 * in the environment). */
typedef enum ndt_handoff_mode { NDT_HANDOFF_ASYNC = 0, NDT_HANDOFF_SYNC = 1 } ndt_handoff_mode;
/* Tuning and A/B switches (round 5).  The production library reads NONE of these from the environment -- a library
 * linked into somebody else's process is not steered by variables that process never heard of.  The environment is
 * left with four documented OPERATIONAL knobs: NDT_HANDOFF=sync (blocking hand-off), NDT_UPLOAD_THREADS (repack
 * workers), NDT_COMM_TIMEOUT_S (multi-rank reduce time-out), NDT_PRELAUNCH=0 (no pre-launched kernels).  Everything
 * else is this struct: process-wide; every field has the default ndt_get_tuning() reports in a fresh process.
 * ndt_set_tuning may be called from any thread at any time: a target build and an evaluation (every evaluation of an
 * align, a batched evaluation) each take ONE copy of the struct when they begin and size and launch everything from
 * that copy, so a call takes effect at the next build / evaluation and never in the middle of one; a kernel
 * pre-launched for the next evaluation keeps the shape it was enqueued with.  mbox_tagged, mbox_preload and
 * prelaunch_streams are read once per handle, at ndt_create.  Results do not depend on any field (same rows, same
 * order, same bits), only timings do -- except deriv_block / deriv_single_level_max, which change the partition of
 * the scan and with it the last bits of the floating-point sums.
 * (The diagnostic library variants -- make VARIANT=ab|seams|stamps -- still take the historical NDT_* variables as
 * initial values of these fields; the tuning programs under tools/ use ndt_set_tuning.) */
typedef struct ndt_tuning {
  int deriv_block;            /* 0: chosen per launch (default); else threads per block of k_derivatives, multiple of 64, 64..1024 */
  int deriv_summer;           /* 1: a fixed block adds the partial rows by polling their tags (default); 0: ticket, last block adds */
  int deriv_dedicated;        /* 1: that block owns no points where a compute unit is spare (default); 0: block 0 doubles */
  int deriv_single_level_max; /* rows one block adds directly (default 2048); larger grids go through 32 group rows */
  int deriv_xcd;              /* 0: chunk = block id; 1: XCD-aware chunks on resident single-pose grids (default); 2: stripes too */
  int bucket_build;           /* 1: steady-state builds in two launches (default); 0: launch-per-phase sort pipeline */
  int bucket_tile;            /* 0: chosen from the cloud size (default); 1024 | 2048 | 4096 | 8192 points per tile of k_bucket_pass */
  int fused_sort;             /* 1: one launch per sort digit where the cloud allows it (default); 0: classic passes */
  int bounds_blocks;          /* blocks of the bounds pass (default 256) */
  int bounds_unroll;          /* 8 (default) | 4 */
  int finalize_threads;       /* 256 (default) | 64 */
  int build_events;           /* -1: HIP events around a build only while kernel timing is on (default); 0 | 1: never | always */
  int build_wait_sync;        /* 0: the host polls the build's done tag (default); 1: hipStreamSynchronize */
  int mbox_tagged;            /* 1: poses reach pre-launched kernels as tagged 8-byte granules (default); 0: words + sequence */
  int mbox_preload;           /* 0 (default); 1: a pre-launched kernel fetches its point before the pose arrives */
  int prelaunch_streams;      /* 2: pre-launched kernels on the engine's second stream (default); 1: one stream */
  int prelaunch_probe;        /* 1: the automatic stream placement probes the other placement (default); 0: never */
  int speculate_first;        /* 1: first evaluation of an align enqueued behind a running build (default); 0: off */
  int timing_bracket;         /* 0: kernel-timing events attached to the dispatch (default); 1: recorded around the launch call */
  int handoff_chunk_pass;     /* 0: the asynchronous host hand-off partitions the target behind its transfer (default); 1: under it, chunk by
                               * chunk on a stream of its own (measured slower: profiles/r05_handoff_chunk_pass_ab.txt) */
  int deriv_summer_split;     /* 1: four summing blocks, one 128-byte line of every row each, where compute units are spare (default); 0: one;
                               * 4 | 8: that many (A/B) */
  int deriv_one_block_per_cu; /* 1: a single-pose launch of at most one block per compute unit asks for more than half a unit's LDS, so that no
                               * two of its blocks share a unit (default); 0: blocks of <= 8 waves may */
  int reserved[10];           /* zero */
} ndt_tuning;
/* Idle-device heartbeat (round 5; default off).  A driver at the reference's 10-20 Hz keyframe rate leaves the device idle for
 * 50-100 ms between two aligns, and an idle MI355X drops its clocks: the align that follows runs 5-10 % slower than in a
 * busy loop.  period_us > 0 (>= 100): while the handle has been idle for a period, a background thread
 * launches one small kernel (one block per compute unit, ~3 us) per period on a lowest-priority stream; 0 stops it.
 * ndt_get_keepwarm returns the period (0: off) and, if beats != NULL, the number of beats launched so far. */
int ndt_set_keepwarm(ndt_handle* h, int period_us);
int ndt_get_keepwarm(const ndt_handle* h, long long* beats);

int ndt_get_tuning(ndt_tuning* out);
/* NDT_ERR_INVALID_ARG (nothing changed) when a field is outside its documented values. */
int ndt_set_tuning(const ndt_tuning* t);

int ndt_set_handoff_mode(ndt_handle* h, int mode);
int ndt_get_handoff_mode(const ndt_handle* h);
/* Blocks until every hand-off in flight is complete on the device; returns the status of a deferred build that
 * failed, NDT_OK otherwise.  A deferred failure is reported once -- by this call or by the first call that needs the
 * grid, whichever comes first; after that the handle is where a failed blocking ndt_set_target leaves it (no target:
 * NDT_ERR_NO_TARGET from the calls that need one). */
int ndt_wait(ndt_handle* h);

/* setInputTarget (ref: run/pipeline.cpp:557): uploads and builds the voxel grid.
 * xyz points to the first x; consecutive points are stride_bytes apart (12 for
 * packed xyz, 32 for pcl::PointXYZI, 16 for pcl::PointXYZ). */
int ndt_set_target(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes);
/* SoA host arrays (LidarFrame x/y/z, ref: include/dataframe.hpp:344-346) */
int ndt_set_target_soa(ndt_handle* h, const float* x, const float* y, const float* z, size_t n);
/* SoA arrays already resident in device memory (consumed during the call) */
int ndt_set_target_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n);
/* As ndt_set_target_device, but under NDT_HANDOFF_ASYNC a steady-state build is only ENQUEUED on the engine's stream:
 * the arrays must stay valid and unchanged until the first call that needs the grid (ndt_align, ndt_get_grid_info,
 * ndt_wait, ...) has returned, and a failed build is reported by that call.  What it buys: the align that follows
 * enqueues its first derivative evaluation BEHIND the build while it still runs (the kernel reads the grid geometry
 * from device memory), so the launch is not paid after the build's verdict -- as for every deferred build: host
 * clouds under NDT_HANDOFF_ASYNC, ndt_set_target_from_keyframes. */
int ndt_set_target_device_deferred(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n);
/* setInputSource (ref: run/pipeline.cpp:558) */
int ndt_set_source(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes);
int ndt_set_source_soa(ndt_handle* h, const float* x, const float* y, const float* z, size_t n);
int ndt_set_source_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n);
/* The same without the copy: the engine reads the caller's device arrays at every later evaluation,
 * so they must stay valid and unchanged until the source is replaced -- pcl::Registration::
 * setInputSource's contract (it keeps the caller's shared_ptr; ref: run/pipeline.cpp:558). */
int ndt_set_source_device_view(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n);
/* The engine may cache a block-ordered COPY of a viewed source (ndt_source_order).  After rewriting
 * the viewed arrays in place (a reused scan buffer) call ndt_set_source_device_view again, or this
 * notice (no copy, no launch): later aligns then re-derive whatever was cached from the arrays.
 * Freeing the arrays while they are the source is the caller's error, as with the shared_ptr. */
int ndt_source_changed(ndt_handle* h);

/* Voxel-record format of the derivative kernel (SURVEY 7 "packed 48-B record").  NDT_RECORDS_F64: 80 bytes per
 * voxel, mean and inverse covariance in f64 (default; what the 1e-9 parity tests run on).  NDT_RECORDS_PACKED48:
 * 48 bytes, the mean stays f64 and the inverse covariance is rounded to f32 -- what the reference's own per-pair
 * gradient / Hessian arithmetic does with it (c_inv4, svn_ndt_impl.hpp:449-456); only the score's Mahalanobis term
 * sees an f32 matrix where the reference keeps f64.  Derivatives move by ~1e-7 of their norm, the aligned transform
 * by micrometres (tests/test_gpu_features.py); an evaluation fetches three 16-byte pieces per neighbour instead of
 * five.  Applies to the DIRECT7 / DIRECT1 neighbourhoods; KDTREE, DIRECT26 and a multi-grid union keep reading the
 * 80-byte records (measured: no gain there; the union chains its leaves through them).  Takes effect at
 * the next evaluation; exported leaf statistics are the f64 ones either way. */
typedef enum ndt_record_format { NDT_RECORDS_F64 = 0, NDT_RECORDS_PACKED48 = 1 } ndt_record_format;
int ndt_set_record_format(ndt_handle* h, int format);
int ndt_get_record_format(const ndt_handle* h);

/* Multi-grid target [RECALLED: tier4 ndt_omp's MultiGridNormalDistributionsTransform -- addTarget /
 * removeTarget / createVoxelKdtree -- named by the reference's build (CMakeLists.txt:41-42); its
 * sources are in the absent extern/ndt_omp submodule and no driver instantiates it].  Every cloud is
 * voxelised on its own (the leaves of setInputTarget on that cloud alone) and kept under an id;
 * ndt_multigrid_create_kdtree makes the union of all stored grids the target: the neighbourhood is
 * the radius search (radius = leaf size) over the centroids of ALL grids' valid leaves, whatever
 * search_method says; a voxel that two grids share contributes once per grid.  Afterwards
 * ndt_align / ndt_score_transform / ndt_eval_derivatives work as after ndt_set_target; a plain
 * ndt_set_target* call replaces the union (the stored grids stay until removed). */
int ndt_multigrid_add_target(ndt_handle* h, int64_t id, const float* xyz, size_t n, size_t stride_bytes);
int ndt_multigrid_remove_target(ndt_handle* h, int64_t id);
int64_t ndt_multigrid_count(const ndt_handle* h);
int ndt_multigrid_create_kdtree(ndt_handle* h);

/* Device-resident keyframe archive + sliding-window target assembly.  The drivers keep every
 * keyframe's body-frame scan (pointsArchive, ref: run/pipeline.cpp:784) and rebuild the NDT
 * target per keyframe as the sum of <= 5 archived scans, each moved by its current pose
 * (ref: run/pipeline_ligo_tc.cpp:519-529; one scan in run/pipeline.cpp:554-557).  Here the
 * scans stay in HBM; only ids and 4x4 double poses cross the boundary per keyframe.
 * Empty keyframes: ndt_keyframe_put accepts n = 0 (xyz may then be NULL).  In a window an empty keyframe adds no
 * point.  A window whose keyframes hold no point at all is NDT_ERR_NO_TARGET, as an empty cloud is for
 * ndt_set_target, and leaves the handle WITHOUT a target (the previous one is not kept).  Viewing an empty keyframe
 * with ndt_set_source_from_keyframe succeeds and leaves the handle without a source, like ndt_set_source_device_view
 * with n = 0: the next call that needs one returns NDT_ERR_NO_SOURCE. */
int ndt_keyframe_put(ndt_handle* h, int64_t id, const float* xyz, size_t n, size_t stride_bytes);
int ndt_keyframe_erase(ndt_handle* h, int64_t id);
int64_t ndt_keyframe_count(const ndt_handle* h);
/* target = concat_k transform(archive[ids[k]], poses16[k]) (f64 transform, rounded to f32 once,
 * as pcl::transformPointCloud with a double matrix), then the voxel-grid build */
int ndt_set_target_from_keyframes(ndt_handle* h, const int64_t* ids, const double* poses16,
                                  int n_keyframes);
/* setInputSource(archive[id]): the scan that was just archived is also the one to register
 * (ref: run/pipeline.cpp:558 registers pointsBody, :784 archives the same cloud) -- one upload
 * serves both.  The source VIEWS the archived scan (no copy): erasing or replacing that keyframe
 * unsets the source (NDT_ERR_NO_SOURCE until one is set again). */
int ndt_set_source_from_keyframe(ndt_handle* h, int64_t id);

/* Deskew (motion compensation) of a scan on the device, from per-point times and a pose trajectory.  The reference
 * computes a per-point interpolation factor pointsAlpha and keeps pointsTimestamp (ref: include/dataframe.hpp:406-433),
 * its sync thread cuts the INS frames of the scan interval into FrameData::ins (ref: run/pipeline.cpp:224-246) and
 * CompFrame::linearInterpolate says how a pose between two frames is meant (position linearly, attitude by slerp, the
 * factor clamped to [0, 1]; ref: include/dataframe.hpp:184-251) -- but no driver reads pointsAlpha: the scan is
 * registered as if taken at one instant.  These calls undo the motion.
 *
 * The model.  A trajectory is n_knots poses, 1 <= n_knots <= NDT_DESKEW_MAX_KNOTS: knot_poses16 holds n_knots 4 x 4
 * doubles, column-major, body -> map at that knot (as ndt_set_target_from_keyframes takes poses); knot_t[n_knots] their
 * times, strictly increasing.  ref_pose16 is the pose the scan is to be expressed in, NULL = the last knot (the drivers
 * take ins.back() and timestamp = end_interval as the frame's pose and time).  Per knot the host forms
 * D_k = ref^-1 T_k in f64 and reduces it to a unit quaternion q_k (sign: q_k . q_{k-1} >= 0) and a translation d_k; a
 * knot whose pose equals the reference bit for bit reduces to the exact identity.  Per segment it computes the
 * half-angle theta_k = atan2(|vec(conj(q_k) q_{k+1})|, scalar part) and 1 / sin(theta_k).  A point with time t:
 *   t is clamped to [knot_t[0], knot_t[n_knots - 1]]; its segment k has knot_t[k] <= t <= knot_t[k + 1];
 *   u = (t - t_k) / (t_{k+1} - t_k) in f64;
 *   q(u) = (sin((1 - u) theta) / sin(theta)) q_k + (sin(u theta) / sin(theta)) q_{k+1}; for theta < 1e-8 the normalised
 *   linear blend; d(u) = d_k + u (d_{k+1} - d_k);
 *   p' = R(q(u)) p + d(u), everything in f64, rounded to f32 once.
 * A segment whose two knots reduce to bit-equal (q, d) is RIGID: the pose is (q_k, d_k) itself and no interpolation
 * arithmetic is applied (n_knots == 1 included).  "No motion" is therefore exact: with every knot equal to the
 * reference every finite point comes back bit for bit.
 * ndt_trajectory_pose (host only: no handle, no device) returns D(t) as the deskew uses it.  NDT_ERR_INVALID_ARG when a
 * pointer is NULL (the reference pose excepted), n_knots is outside 1 .. 64, knot_t is not strictly increasing, or a
 * knot time, a pose entry or t is not finite. */
#define NDT_DESKEW_MAX_KNOTS 64
int ndt_trajectory_pose(const double* knot_t, const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
                        double t, double out_pose16[16]);
/* The acquisition filter of the drivers' lidar callback, applied to the RAW coordinates in the same pass (sensor frame,
 * as at capture; ref: src/lidarcallback.cpp:533-538):
 *   keep = finite(x, y, z, t)
 *       && !(use_box && box_min[a] <= p[a] <= box_max[a] on all three axes)
 *       && (!use_z_or_intensity || (z_min <= z && z <= z_max)
 *           || (intensity != NULL && intensity[i] >= intensity_keep_min))
 * A zeroed struct keeps every finite point (a compaction of the NaN returns). */
typedef struct ndt_scan_filter {
  int use_box;              float box_min[3], box_max[3];           /* vehicleFilterBox: centre -/+ dimensions / 2 */
  int use_z_or_intensity;   float z_min, z_max, intensity_keep_min; /* zAxisFilter, reflectivity threshold */
} ndt_scan_filter;
/* ndt_deskew_device: SoA float arrays in device memory in and out; d_t is one float per point in the units of knot_t
 * (pointsAlpha with knots at normalised times, or LidarFrame::relative_timestamp with knots at
 * ins[k].timestamp_20 - frame.timestamp).  d_intensity, o_intensity and d_index_out may be NULL (an intensity output
 * needs an intensity input); d_intensity == NULL with use_z_or_intensity set is valid, the second alternative is then
 * false for every point.  n <= INT32_MAX; n = 0 is a no-op with *n_out = 0.
 *  - filter_or_null == NULL (aligned): one launch, out[i] is the deskewed in[i], a point whose t or coordinates are not
 *    finite gives NaN in x, y and z; *n_out = n; cap >= n (NDT_ERR_INVALID_ARG otherwise, nothing written).  An output
 *    may BE an input array (the same address: in place); any other overlap of an output with an input is refused.
 *  - filter_or_null != NULL (compacting): the kept points, deskewed, densely and in input order (the three launches of
 *    ndt_filter_source's compaction: ballots, one block scanning the block counts, emit; integer offsets, no atomics).
 *    At most cap points are written, *n_out is the number selected, NDT_ERR_INVALID_ARG naming it if it exceeds cap
 *    (cap = n always suffices).  d_index_out receives each kept point's position in the input.  No output may
 *    overlap an input (NDT_ERR_INVALID_ARG).
 * Everything runs on the engine's stream and is complete when the call returns.  The handle's target, source, align
 * state, iteration history, evaluation counters, map and archive are left alone.  An argument error refuses the call as
 * a whole: nothing is written. */
int ndt_deskew_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, const float* d_intensity,
                      const float* d_t, size_t n, const double* knot_t, const double* knot_poses16, int n_knots,
                      const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* ox, float* oy, float* oz,
                      float* o_intensity, int32_t* d_index_out, size_t cap, size_t* n_out);
/* host form: a strided cloud in (stride_bytes apart; intensity at intensity_offset_bytes, < 0: none -- pcl::PointXYZI:
 * stride 32, intensity at 16), t contiguous (n floats); out: a cloud of the same layout, of which x, y, z and the
 * intensity of the first *n_out points are written (nothing if *n_out exceeds cap); index_out (nullable): n_out ints */
int ndt_deskew(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, long intensity_offset_bytes, const float* t,
               const double* knot_t, const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
               const ndt_scan_filter* filter_or_null, float* out, int32_t* index_out, size_t cap, size_t* n_out);
/* ndt_keyframe_put of the deskewed (and, with a filter, compacted) scan: the archive holds under `id` exactly what
 * ndt_keyframe_put would hold for the output of ndt_deskew -- replaced-keyframe and viewed-source rules and the buffer
 * pool included -- so ndt_set_source_from_keyframe(id) and ndt_map_add_keyframe work on it: one upload serves the source
 * and the archive (ref: run/pipeline.cpp:558,784).  *n_kept (nullable) receives the number of points archived.  An
 * argument error leaves the archive untouched. */
int ndt_keyframe_put_deskewed(ndt_handle* h, int64_t id, const float* xyz, size_t n, size_t stride_bytes,
                              long intensity_offset_bytes, const float* t, const double* knot_t, const double* knot_poses16,
                              int n_knots, const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null,
                              size_t* n_kept);

/* Unprojection of a lidar range image on the device, fused with the acquisition filter and the deskew.  The drivers'
 * lidar callback turns every pixel of the range image into a point with one multiply-add per coordinate against a
 * lookup table (ref: src/lidarcallback.cpp:191-327 builds it, :455-545 and :570-610 use it), applies the range filter
 * and the acquisition filter and pushes the point; these calls take the range image as received -- a 20-bit range in
 * millimetres and one reflectivity byte per pixel, one time per column, column by column -- and return the filtered,
 * deskewed, compacted scan (or, without a filter, the organised cloud).  Packet parsing stays with the driver (or goes
 * to the device as well: ndt_packet_frame_push and ndt_unproject_packet_frame* below take the UDP payloads).
 *
 * The scan model: the unprojection tables of the lidar callback (ref: src/lidarcallback.cpp:286-327):
 *   p = range_m * (x1,y1,z1)[col * n_rows + row] + (x2,y2,z2)[col]
 * x1,y1,z1: n_cols*n_rows floats each; x2,y2,z2: n_cols floats each; host pointers, copied to the device and kept
 * until replaced, cleared or the handle is destroyed.  1 <= n_rows, 1 <= n_cols, n_cols*n_rows <= INT32_MAX.
 * ndt_scan_model_get_info returns 0, 0 when none is set. */
int ndt_scan_model_set(ndt_handle* h, int n_cols, int n_rows, const float* x1, const float* y1, const float* z1,
                       const float* x2, const float* y2, const float* z2);
int ndt_scan_model_clear(ndt_handle* h);
int ndt_scan_model_get_info(const ndt_handle* h, int* n_cols, int* n_rows);
/* host only, no handle, no device: the tables as the callback's Initialize() computes them, in its arithmetic (float
 * angles, float sin/cos, the 4x4 lidar->body transform in double, one rounding to float):
 *   azimuth of column m = 2 pi (1 - m / n_cols) + beam azimuth of the row; direction = lidar_to_body's rotation applied
 *   to (cos alt cos az, cos alt sin az, sin alt); offset = lidar_to_body applied to (r0 cos az_m, r0 sin az_m, 0, 1) with
 *   r0 = lidar_origin_to_beam_origin_mm / 1000.
 * n_rows beam angles each, in degrees.  NDT_ERR_INVALID_ARG when a pointer is NULL, a size is below 1, n_cols*n_rows
 * exceeds INT32_MAX or an angle, the beam origin or a transform entry is not finite; nothing is written then. */
int ndt_scan_model_from_beams(int n_cols, int n_rows, const float* beam_azimuth_deg, const float* beam_altitude_deg,
                              double lidar_origin_to_beam_origin_mm, const double lidar_to_body16_colmajor[16],
                              float* x1, float* y1, float* z1, float* x2, float* y2, float* z2);
typedef struct ndt_range_gate {
  int use_range;  float range_min, range_max;   /* rangeFilter, metres, inclusive (ref: :531, :575) */
  int row_step;                                 /* channel stride: only rows with row % row_step == 0; 0 or 1 = all */
} ndt_range_gate;
/* Per pixel i = col * n_rows + row of the range image (gate_or_null == NULL: no range filter, every row):
 *   valid = range_mm[i] != 0 && row % row_step == 0 && finite(col_t[col])
 *           && (!use_range || (range_min <= range_m && range_m <= range_max))
 *           (a non-finite column time marks a column that never arrived);
 *   range_m = (float)range_mm[i] * 0.001f, one f32 multiply;
 *   x = fmaf(range_m, x1[i], x2[col]), y and z likewise: a fused multiply-add with a single rounding, as the
 *           reference's AVX path computes it (ref: :512-514), whatever the compiler's contraction setting;
 *   intensity = (float)reflectivity[i], t = col_t[col];
 *   n_knots > 0: the point is moved exactly as ndt_deskew moves (x, y, z, t) -- the same trajectory model, the same
 *           ref_pose16_or_null, the same rigid-segment and exact-identity rules; n_knots == 0 with knot_t, knot_poses16
 *           and ref_pose16_or_null NULL: no motion, the raw point comes out;
 *   filter_or_null != NULL: ndt_scan_filter on the RAW (x, y, z) with (float)reflectivity as the intensity (none
 *           without a reflectivity array) -- exactly the predicate of ndt_deskew.
 * ndt_unproject_device: d_range_mm (n_cols*n_rows uint32), d_reflectivity (n_cols*n_rows bytes, nullable), d_col_t
 * (n_cols floats) and every output in device memory; o_intensity, o_t and d_index_out are nullable (o_intensity needs
 * d_reflectivity); d_index_out receives the pixel index i.
 *  - filter_or_null == NULL (organised): one launch, out[i] is pixel i, an invalid pixel gives NaN in x, y and z,
 *    intensity and t are written as they are; *n_out = n_cols*n_rows; cap >= that (NDT_ERR_INVALID_ARG otherwise).
 *  - filter_or_null != NULL (compacting): the valid, kept points densely and in pixel order, the order in which the
 *    reference's decode pushes them (the three launches of ndt_deskew's compaction: ballots, one block scanning the
 *    block counts, emit; integer offsets, no atomics).  A zeroed filter drops only the invalid pixels.  At most cap
 *    points are written, *n_out is the number selected, NDT_ERR_INVALID_ARG naming it if it exceeds cap.
 * Any overlap of an output with an input, or of two outputs with each other, is refused (the outputs are distinct
 * arrays).  NDT_ERR_INVALID_ARG also when no model is set, a required
 * pointer is NULL, row_step is negative, use_range is set with range_min > range_max (or a NaN bound), or the
 * trajectory is refused by the rules of ndt_deskew.  Everything runs on the engine's stream and is complete when the
 * call returns.  The handle's target, source, align state, iteration history, evaluation counters, map and archive are
 * left alone.  An argument error refuses the call as a whole: nothing is written. */
int ndt_unproject_device(ndt_handle* h, const uint32_t* d_range_mm, const uint8_t* d_reflectivity, const float* d_col_t,
                         const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16, int n_knots,
                         const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* ox, float* oy,
                         float* oz, float* o_intensity, float* o_t, int32_t* d_index_out, size_t cap, size_t* n_out);
/* host form: range_mm (n_cols*n_rows uint32), reflectivity (n_cols*n_rows bytes, nullable) and col_t (n_cols floats)
 * are contiguous host arrays and go up through pinned staging in ONE transfer; out: a strided cloud laid out as
 * ndt_deskew's (x, y, z and, with intensity_offset_bytes >= 0 -- which needs reflectivity --, the intensity of the
 * first *n_out points are written; nothing if *n_out exceeds cap); t_out (nullable): n_out floats; index_out
 * (nullable): n_out ints. */
int ndt_unproject(ndt_handle* h, const uint32_t* range_mm, const uint8_t* reflectivity, const float* col_t,
                  const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16, int n_knots,
                  const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* out, size_t stride_bytes,
                  long intensity_offset_bytes, float* t_out, int32_t* index_out, size_t cap, size_t* n_out);
/* ndt_keyframe_put of the compacting output: the archive holds under `id` exactly what ndt_keyframe_put would hold for
 * it -- replaced-keyframe and viewed-source rules and the buffer pool as in ndt_keyframe_put_deskewed -- so
 * ndt_set_source_from_keyframe(id) and ndt_map_add_keyframe work on it: one upload of 5 bytes per pixel serves the
 * source, the archive and the map.  filter_or_null == NULL means the zeroed filter here (an archive holds no NaN
 * points).  *n_kept (nullable) receives the number of points archived.  An argument error leaves the archive untouched. */
int ndt_keyframe_put_from_ranges(ndt_handle* h, int64_t id, const uint32_t* range_mm, const uint8_t* reflectivity,
                                 const float* col_t, const ndt_range_gate* gate_or_null, const double* knot_t,
                                 const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
                                 const ndt_scan_filter* filter_or_null, size_t* n_kept);

/* Lidar packets decoded on the device: the UDP payloads as the socket delivered them (the reference's DataBuffer) to the
 * range image and on to the deskewed scan.  The host reads the packet and column HEADERS only; a kernel gathers the
 * pixels (ref: src/lidarcallback.cpp:382-891 walks every pixel on the host).  n_cols (columns per frame) and n_rows
 * (pixels per column) are the scan model's; columns_per_packet (cpp) >= 1 is the caller's.
 *
 *                              NDT_LIDAR_PROFILE_RNG19 (RNG19_RFL8_SIG16_NIR16)   NDT_LIDAR_PROFILE_LEGACY
 *   packet header / footer     32 / 32 bytes                                      0 / 0
 *   column header              12 bytes                                           16 bytes
 *   per-column trailer         none                                               4-byte block status
 *   block (one column)         12 + 12*n_rows                                     16 + 12*n_rows + 4
 *   packet size                64 + cpp*block                                     cpp*block
 *   packet accepted when       size matches and LE u16 at byte 0 is 0x0001        size matches
 *   packet frame id            LE u16 at byte 2                                   LE u16 at byte 10 of its FIRST column
 *   column timestamp           LE u64 ns at block+0                               LE u64 ns at block+0
 *   column m_id                LE u16 at block+8                                  LE u16 at block+8
 *   column valid when          byte[block+10] & 1                                 LE u32 at block+16+12*n_rows is 0xFFFFFFFF
 *                                                                                 and LE u16 at block+10 is the packet frame id
 *   first pixel at             block+12                                           block+16
 *   pixel: 12 bytes, LE dwords d0 d1 d2
 *     range_mm                 d0 & 0x0007FFFF                                    d0 & 0x000FFFFF
 *     reflectivity, signal, nir   d1 & 0xFF, d1 >> 16, d2 & 0xFFFF (both)
 * A column whose m_id is not below n_cols is rejected (checked first; then, LEGACY, the frame id; then the status).
 * Every offset is a multiple of 4: the packed packet buffer keeps each accepted packet, in arrival order, at a stride of
 * the packet size rounded up to 16 bytes, and the kernel uses dword loads only.
 * Column time: ts = fmod((double)timestamp_ns * 1e-9, 86400.0); col_t[m] = (float)max(0.0, ts - t_ref), one rounding; a
 * column that never arrived or was rejected has col_t = NaN (and the validity rule of ndt_unproject* drops its pixels).
 * t_ref is the caller's when it is finite, otherwise the ts of the first accepted column in arrival order (the
 * reference's active_frame_->timestamp whenever that column holds a kept point).
 * Two deviations from the reference: it pushes points in arrival order and would push a duplicated column twice -- an
 * image holds one column per m_id; when an m_id arrives more than once the LAST arrival holds (decided on the host).
 * A frame holds at most 2 * ceil(n_cols / cpp) accepted packets. */
#define NDT_LIDAR_PROFILE_RNG19 0
#define NDT_LIDAR_PROFILE_LEGACY 1
typedef struct ndt_packet_frame_info {
  int32_t frame_id;                /* of the first accepted packet; -1: none yet */
  int32_t next_frame_pending;      /* a packet of another frame id stopped the last push */
  double t_ref;                    /* the reference time in use; NaN: automatic and no column accepted yet */
  double ts_first, ts_last;        /* ts of the first and the latest accepted column in arrival order; NaN: none */
  int64_t n_columns;               /* image columns that hold an arrival */
  int64_t n_packets;               /* packets taken, the rejected ones included */
  int64_t n_packets_accepted;      /* ... of which accepted = slots of the packed buffer in use */
  int64_t n_packets_bad_size, n_packets_bad_type;
  int64_t n_columns_bad_id, n_columns_bad_frame, n_columns_bad_status;
  int64_t n_columns_overridden;    /* arrivals of an m_id that already held a column */
} ndt_packet_frame_info;
/* host only, no handle, no device: the whole host pre-pass.  packets: n_packets payloads stride_bytes apart, packet k
 * being bytes_each[k] bytes long; taken in order until one carries another frame id than the first accepted one
 * (info->next_frame_pending, that packet is not taken) or the frame's capacity is used up.  col_src[n_cols]: the DWORD
 * offset of the column's first pixel inside the packed packet buffer, -1 where no column holds; col_t[n_cols] as above;
 * t_ref NaN: automatic.  NDT_ERR_INVALID_ARG when an output pointer is NULL, packets or bytes_each is NULL with
 * n_packets > 0, the profile is unknown, a count is below 1, the packed buffer would exceed 2^31 dwords, t_ref is
 * infinite or a bytes_each[k] exceeds stride_bytes; nothing is written then. */
int ndt_packet_columns(int profile, int columns_per_packet, int n_cols, int n_rows, const uint8_t* packets,
                       const size_t* bytes_each, size_t n_packets, size_t stride_bytes, double t_ref, int32_t* col_src,
                       float* col_t, ndt_packet_frame_info* info);
/* The format of the handle's packets; needs a scan model (its n_cols and n_rows).  ndt_scan_model_set and
 * ndt_scan_model_clear drop the format and any frame in progress.  ndt_packet_format_get: *profile = -1 when none is
 * set.  ndt_packet_size: the payload size that is accepted, 0 when no format is set. */
int ndt_packet_format_set(ndt_handle* h, int profile, int columns_per_packet);
int ndt_packet_format_get(const ndt_handle* h, int* profile, int* columns_per_packet);
size_t ndt_packet_size(const ndt_handle* h);
/* A frame, packet by packet.  ndt_packet_frame_begin waits for the engine's stream and forgets the frame in progress.
 * ndt_packet_frame_push takes n_packets payloads in order (layout as ndt_packet_columns takes them): the first accepted
 * packet fixes the frame id; a packet with another frame id stops the call -- *n_taken < n_packets, NDT_OK,
 * next_frame_pending = 1: finish the frame, call begin and push that packet again (the reference's completion rule).
 * Rejected packets count as taken.  Each accepted packet is copied into its own slot of a pinned staging area and the
 * call's slots go to the device packet buffer with one asynchronous copy on the engine's stream: a push returns without
 * waiting, no slot is reused before the next begin.  One accepted packet more than the capacity is
 * NDT_ERR_INVALID_ARG ("frame overfull") with nothing of that call taken and the frame in progress as it was.
 * ndt_packet_frame_get_info: the counters of the frame in progress. */
int ndt_packet_frame_begin(ndt_handle* h);
int ndt_packet_frame_push(ndt_handle* h, const uint8_t* packets, const size_t* bytes_each, size_t n_packets, size_t stride_bytes,
                          size_t* n_taken);
int ndt_packet_frame_get_info(const ndt_handle* h, ndt_packet_frame_info* info);
/* The range image of the frame in progress into caller-owned DEVICE memory: d_range_mm (n_cols*n_rows uint32),
 * d_reflectivity (n_cols*n_rows bytes, nullable), d_signal and d_nir (n_cols*n_rows uint16, nullable), d_col_t (n_cols
 * floats); pixel i = col * n_rows + row, a column that does not hold is zeros with col_t = NaN.  One launch of
 * k_decode_packets; complete on return.  The frame stays in progress: more packets may follow and be decoded again. */
int ndt_decode_packet_frame_device(ndt_handle* h, uint32_t* d_range_mm, uint8_t* d_reflectivity, uint16_t* d_signal,
                                   uint16_t* d_nir, float* d_col_t);
/* ndt_unproject_device, ndt_unproject and ndt_keyframe_put_from_ranges on the frame in progress: the image is decoded
 * into the handle's scratch and goes through the same launches, so every output is bit for bit what those calls return
 * for the decoded image (reflectivity always present).  signal_out / nir_out (nullable, uint16; device memory in the
 * _device form, host memory otherwise): signal and nir of the points written, in their order -- in the compacting form
 * gathered through the pixel index by a second small kernel; cap elements (the keyframe form: n_cols*n_rows).
 * Refused, with nothing written and the cause in ndt_last_error: no scan model, no packet format, no accepted column,
 * signal_out / nir_out overlapping another output, and every refusal of the call it stands for.  The handle's target,
 * source, align state, map and archive are left alone, except the archive entry being put.  Complete on return. */
int ndt_unproject_packet_frame_device(ndt_handle* h, const ndt_range_gate* gate_or_null, const double* knot_t,
                                      const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
                                      const ndt_scan_filter* filter_or_null, float* ox, float* oy, float* oz, float* o_intensity,
                                      float* o_t, int32_t* d_index_out, uint16_t* d_signal_out, uint16_t* d_nir_out, size_t cap,
                                      size_t* n_out);
int ndt_unproject_packet_frame(ndt_handle* h, const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16,
                               int n_knots, const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* out,
                               size_t stride_bytes, long intensity_offset_bytes, float* t_out, int32_t* index_out,
                               uint16_t* signal_out, uint16_t* nir_out, size_t cap, size_t* n_out);
int ndt_keyframe_put_from_packets(ndt_handle* h, int64_t id, const ndt_range_gate* gate_or_null, const double* knot_t,
                                  const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
                                  const ndt_scan_filter* filter_or_null, uint16_t* signal_out, uint16_t* nir_out, size_t* n_kept);

/* pcl::VoxelGrid downsample on the device (ref: run/pipeline_ins_map_distribution.cpp:324-340: the accumulated map
 * is filtered at `mapvoxelsize` before the NDT export).  PCL's published algorithm: the grid of
 * getMinMax3D over the finite points, voxel index floor(p * inv_leaf) - min_b, every field averaged (in float) over
 * the points of an occupied voxel, output in ascending voxel index; non-finite points are dropped; a grid of more than
 * INT32_MAX cells is refused (NDT_ERR_GRID_OVERFLOW).  Within a voxel the points are added in input order.
 *  - _device: SoA float arrays in device memory in and out (intensity arrays may be NULL); at most `cap` points are
 *    written, *n_out receives the number of occupied voxels (NDT_ERR_INVALID_ARG if it exceeds cap; cap = n always
 *    suffices).  The output arrays can go straight into ndt_set_target_device: no host round trip.
 *  - host form: a strided cloud in (stride_bytes apart; intensity at intensity_offset_bytes, < 0: none --
 *    pcl::PointXYZI: stride 32, intensity at 16) and a cloud of the same layout out (only x, y, z and intensity are
 *    written).
 * The handle's target grid and source are left untouched. */
int ndt_voxel_downsample_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, const float* d_intensity,
                                size_t n, float leaf, float* ox, float* oy, float* oz, float* o_intensity, size_t cap,
                                size_t* n_out);
int ndt_voxel_downsample(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, long intensity_offset_bytes,
                         float leaf, float* out, size_t cap, size_t* n_out);

/* Sparse voxel map accumulated scan by scan (ref: run/pipeline_ins_map_distribution.cpp:281-377: the map driver moves
 * every keyframe scan into the map frame, keeps all of them, and at shutdown filters the concatenation with
 * pcl::VoxelGrid(mapvoxelsize), builds the NDT grid from the result and exports the leaves).  Here one map per handle
 * lives in device memory and holds, per occupied voxel, the float sums of x, y, z (and intensity) and an int32 count:
 * the points are not kept, there is no dense index (ndt_voxel_downsample refuses a bounding box of more than INT32_MAX
 * cells; the map does not care how far apart its voxels are), and the map built so far can be exported or made the
 * target at any time.  The export is bit for bit what ndt_voxel_downsample returns for the concatenation of everything
 * added, wherever that call is possible: a voxel is floor(p * inv_leaf) per axis in f32 (inv_leaf = 1.0f / leaf)
 * whatever the bounding box is, a voxel's points are added one at a time in input order, continuing from the sums the
 * map holds, and the output is in ascending (k, j, i) order, which is PCL's ascending voxel index.
 *  - ndt_map_reset: a new, empty map (an existing one is freed).  leaf > 1e-6f; initial_capacity: table slots to start
 *    with (rounded up to a power of two; 0: the default, 2^18).  The table grows by itself: after every add it holds at
 *    most capacity / 2 voxels.
 *  - ndt_map_clear frees the map; the other ndt_map_* calls and ndt_set_target_from_map then return
 *    NDT_ERR_INVALID_ARG ("no map").
 *  - ndt_map_add / _device / _keyframe: one cloud -- a strided host cloud (as ndt_voxel_downsample takes it), SoA arrays
 *    in device memory, or an archived keyframe -- moved by a 4x4 double pose (column-major; NULL: as it is; f64 products
 *    summed left to right, rounded to f32 once, as ndt_set_target_from_keyframes moves a scan).  Non-finite points,
 *    before or after the pose, are skipped and counted.  Voxel coordinates are limited to |ijk| < 2^20 per axis: an add
 *    with a finite point beyond is refused as a whole (NDT_ERR_GRID_OVERFLOW); so is one the table cannot grow for
 *    (NDT_ERR_ALLOC).  Both are decided before anything is written: the map is unchanged.  n = 0 is a no-op.  A map
 *    created with intensity needs it in every add (intensity_offset_bytes < 0, d_intensity == NULL or a keyframe, which
 *    holds xyz only: NDT_ERR_INVALID_ARG); one created without ignores it.  The caller's arrays are free when the call
 *    returns.
 *  - ndt_map_export / _device: one point per voxel with count >= min_points (<= 1: all; PCL's
 *    setMinimumPointsNumberPerVoxel), every field sum / (float)count.  At most `cap` points are written, *n_out
 *    receives the number selected (NDT_ERR_INVALID_ARG naming it if it exceeds cap); o_intensity, o_count / count_out
 *    may be NULL (count_out: `cap` contiguous int32).  Complete when it returns; the map is unchanged and can be added
 *    to afterwards.
 *  - ndt_set_target_from_map: the export with min_points becomes the target (the driver's line 368), without a host
 *    round trip; the build is reported and deferred as ndt_set_target_from_keyframes' is.  An empty selection is
 *    NDT_ERR_NO_TARGET and leaves the target as it was.
 * Target grid, source, align state, iteration history, evaluation counters and the keyframe archive are left untouched
 * by the ndt_map_* calls; the map survives ndt_set_target* and ndt_set_params and is freed by ndt_map_clear, a new
 * ndt_map_reset or ndt_destroy. */
typedef struct ndt_map_info {
  float leaf;
  int with_intensity;
  int64_t n_voxels;          /* occupied voxels */
  int64_t n_points;          /* finite points accumulated */
  int64_t n_points_dropped;  /* non-finite points skipped */
  int64_t capacity;          /* table slots (power of two) */
  int min_ijk[3], max_ijk[3];/* absolute voxel coordinates; undefined when n_voxels == 0 */
  int64_t n_adds, n_grows;
} ndt_map_info;
int ndt_map_reset(ndt_handle* h, float leaf, int with_intensity, int64_t initial_capacity);
int ndt_map_clear(ndt_handle* h);
int ndt_map_add(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, long intensity_offset_bytes,
                const double* pose16_colmajor_or_null);
int ndt_map_add_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, const float* d_intensity,
                       size_t n, const double* pose16_colmajor_or_null);
int ndt_map_add_keyframe(ndt_handle* h, int64_t id, const double pose16_colmajor[16]);
int ndt_map_get_info(const ndt_handle* h, ndt_map_info* out);
int ndt_map_export_device(ndt_handle* h, int min_points, float* ox, float* oy, float* oz, float* o_intensity,
                          int32_t* o_count, size_t cap, size_t* n_out);
int ndt_map_export(ndt_handle* h, int min_points, float* out, size_t stride_bytes, long intensity_offset_bytes,
                   int32_t* count_out, size_t cap, size_t* n_out);
int ndt_set_target_from_map(ndt_handle* h, int min_points);

/* Per-voxel moments and the NDT target made from them (the classical NDT map).  ndt_set_target_from_map builds the
 * target from one centroid per map voxel, as the driver's shutdown code does: the distribution of the points inside a
 * voxel is lost, and the whole map has to fit one dense index.  With moments on, the map keeps per voxel the nine sums
 * the target build reduces a voxel's points to -- sum x, y, z and sum xx, xy, xz, yy, yz, zz, in f64 of the f32
 * coordinates, one point at a time in input order, continuing from what the map holds (the order of the reference's
 * own loop, so the sums do not depend on how the points were split into adds) -- and the leaves are made from them.
 *  - ndt_map_enable_moments: allowed on a map that has accumulated no point yet (right after ndt_map_reset), once;
 *    otherwise NDT_ERR_INVALID_ARG.  Every later add also accumulates the moments (72 more bytes per voxel).  A new
 *    ndt_map_reset gives a map without moments.  ndt_map_has_moments: 1 / 0 (0 without a map).  The other ndt_map_*
 *    calls and ndt_set_target_from_map behave, bit for bit, as on a map without moments.
 *  - ndt_map_export_moments: host arrays (any may be NULL) of the voxels with count >= min_points in ascending
 *    (k, j, i) order: ijk 3 ints, count, sums 9 doubles {x, y, z, xx, xy, xz, yy, yz, zz} per voxel.  Size protocol
 *    as ndt_map_export.  NDT_ERR_INVALID_ARG on a map without moments.
 *  - ndt_set_target_from_map_moments: box_min / box_max both NULL: the whole map; otherwise the voxels with
 *    floor(box_min[a] * inv_leaf) <= ijk[a] <= floor(box_max[a] * inv_leaf) on every axis (the f32 floor of a point's
 *    voxel).  The target becomes what ndt_set_target would build, under the handle's current ndt_params, from the
 *    finite points ever added whose voxel is inside the box: the grid geometry is the ijk box of the occupied voxels
 *    selected, the leaves are those with at least max(3, min_points_per_voxel) points, n_target_points is the sum of
 *    the selected voxels' counts.  Leaf slots are handed out in ascending voxel order: two handles fed the same adds
 *    hold the same table.  Refusals, each leaving the target exactly as it was: no map, no moments, a map leaf that is
 *    not bit-equal to ndt_params::resolution, a box that is not finite or given by halves (NDT_ERR_INVALID_ARG); no
 *    occupied voxel selected (NDT_ERR_NO_TARGET); a selected ijk box of INT32_MAX cells or more
 *    (NDT_ERR_GRID_OVERFLOW).  The call completes before it returns.  Afterwards the handle is where
 *    ndt_set_target_device leaves it: no target points are retained (ndt_fitness_score: NDT_ERR_UNSUPPORTED; an
 *    ndt_set_params that changes the grid drops it until this function is called again -- the map is still there). */
int ndt_map_enable_moments(ndt_handle* h);
int ndt_map_has_moments(const ndt_handle* h);
int ndt_map_export_moments(ndt_handle* h, int min_points, int32_t* ijk, int32_t* count, double* sums, size_t cap,
                           size_t* n_out);
int ndt_set_target_from_map_moments(ndt_handle* h, const float box_min[3], const float box_max[3]);

/* Bound, keep and combine a map: remove voxels by box, hand out and take back the complete state of its voxels.  A box
 * is what ndt_set_target_from_map_moments takes: a voxel is inside when floor(box_min[a] * inv_leaf) <= ijk[a] <=
 * floor(box_max[a] * inv_leaf) on every axis (f32 floor, held to the map's coordinate range); box_min[a] > box_max[a]
 * on an axis is an empty box and valid.  File formats stay the caller's business.
 *  - ndt_map_crop: remove_inside == 0 keeps the voxels inside the box and drops the rest (a sliding window around the
 *    vehicle; an empty box empties the map), != 0 drops the voxels inside (erase a region).  *n_removed (nullable):
 *    voxels dropped.  Nothing to drop: NDT_OK, the table untouched.  Otherwise the survivors move, bit for bit, into a
 *    fresh table of the smallest power-of-two capacity >= 2 x kept that is not below the capacity ndt_map_reset gave
 *    the map, and the old table is freed; an allocation failure is NDT_ERR_ALLOC and leaves the map as it was.
 *    Afterwards ndt_map_get_info reports n_voxels and n_points of what was kept, the TIGHT min_ijk / max_ijk of the kept
 *    voxels and the new capacity; n_points_dropped, n_adds and n_grows are unchanged.  An emptied map still exists and
 *    keeps its moments setting.  Both box pointers are needed and every value finite (NDT_ERR_INVALID_ARG).
 *  - ndt_map_export_state / _device: every OCCUPIED voxel of the map (both box pointers NULL) or of a box, in ascending
 *    (k, j, i) order: ijk 3 x int32, count int32, sums4 4 x float {sum x, sum y, sum z, sum intensity (0 in a map
 *    without)} exactly as the table holds them (NOT divided by the count), moments9 9 x double as
 *    ndt_map_export_moments gives them.  Any output may be NULL; moments9 != NULL on a map without moments, half a box
 *    or a non-finite box is NDT_ERR_INVALID_ARG.  Size protocol of ndt_map_export.  Complete when it returns; the map is
 *    unchanged.
 *  - ndt_map_import_state / _device: n such records are merged into the map through the add's own pipeline.  Per voxel,
 *    for its records in input order: every sum = what the map holds + the record's sum, rounded once (f32 for sums4,
 *    intensity only in a map with intensity; f64 for moments9), count += the record's count.  A voxel new to the map
 *    starts from +0 and so receives its record bit for bit (0 + s is s for every value but -0.0, which a map never
 *    holds and never exports): export -> import into an empty map restores the state exactly, and a map that is saved,
 *    loaded and continued holds what it would hold had it never stopped.  For a voxel both sides hold, the merged sums
 *    differ from those of one map fed all the points by that one rounding per field.  Refusals, each as a whole with the
 *    map unchanged: no map, NULL ijk / count / sums4, a leaf that is not bit-equal to the map's, moments9 == NULL on a
 *    map with moments (one without ignores moments9), any count < 1 (NDT_ERR_INVALID_ARG, the message names how many);
 *    any |ijk| >= 2^20 (NDT_ERR_GRID_OVERFLOW); a table that cannot grow to 2 x (n_voxels + n) slots (NDT_ERR_ALLOC).
 *    n = 0 is a no-op.  On success n_points grows by the sum of the counts, min_ijk / max_ijk widen, n_adds grows by 1.
 *    The sums are NOT checked for finiteness, and keeping a voxel's int32 count in range is the caller's business, as
 *    it is for ndt_map_add.  The caller's arrays are free when the call returns.
 * The target (also one made from this map before), source, align state, iteration history, evaluation counters and
 * the keyframe archive are left untouched by all five calls. */
int ndt_map_crop(ndt_handle* h, const float box_min[3], const float box_max[3], int remove_inside, int64_t* n_removed);
int ndt_map_export_state(ndt_handle* h, const float box_min[3], const float box_max[3], int32_t* ijk, int32_t* count,
                         float* sums4, double* moments9, size_t cap, size_t* n_out);
int ndt_map_export_state_device(ndt_handle* h, const float box_min[3], const float box_max[3], int32_t* ijk,
                                int32_t* count, float* sums4, double* moments9, size_t cap, size_t* n_out);
int ndt_map_import_state(ndt_handle* h, float leaf, const int32_t* ijk, const int32_t* count, const float* sums4,
                         const double* moments9, size_t n);
int ndt_map_import_state_device(ndt_handle* h, float leaf, const int32_t* ijk, const int32_t* count, const float* sums4,
                                const double* moments9, size_t n);

/* Free-space carving: drop the map voxels that a later scan looks straight through (NDT-OM).  ndt_map_add only gains
 * evidence and ndt_map_crop removes by position; a map kept for hours otherwise fills with the trails of everything
 * that moved, and ndt_set_target_from_map* turns the trails into leaves.  A measured ray from the sensor to a return
 * says that every voxel it crosses before the return is empty now.  One call takes one scan -- a strided host cloud,
 * SoA arrays in device memory or an archived keyframe -- and `origin`, the sensor position in the cloud's own frame;
 * the pose (NULL: none) moves the origin together with the points.
 *  1. Frame.  Points and origin are moved by the pose exactly as ndt_map_add moves a point: f64 products summed left to
 *     right, rounded to f32 once; with a NULL pose they are taken as they are.  Per axis g = (double)(p_f32 *
 *     inv_leaf_f32): the f32 product the add floors, widened to f64.  The start voxel is vs = floor(gs) of the origin,
 *     the end voxel ve = floor(ge) of the point: a ray ends in exactly the voxel ndt_map_add would put its point in.
 *  2. Skipped rays, counted in n_rays_skipped: a point that is not finite, before or after the pose; |vs| or |ve|
 *     reaching 2^20 on an axis.  An origin that is not finite (also: behind the pose) is NDT_ERR_INVALID_ARG.
 *  3. Traversal: Amanatides-Woo in f64 in voxel units, every operation rounded as written, IEEE division.  d = ge - gs.
 *     Per axis with ve[a] != vs[a]: step = +-1, tDelta = 1.0 / fabs(d), tMax = ((double)(vs + (step > 0 ? 1 : 0)) - gs)
 *     / d.  An axis with v[a] == ve[a], initially or once reached, has tMax = +inf.  Each step advances the axis with the
 *     smallest tMax, the lowest axis index on equal values: v[a] += step; tMax[a] += tDelta[a].  The path v_0 = vs ..
 *     v_L = ve therefore has exactly L = |ve - vs|_1 steps.
 *  4. Marks.  A miss goes to v_i for 1 <= i <= min(L - 1 - keep_last, max_steps) (none when that bound is below 1), a
 *     hit goes to v_L whatever L is.  Only voxels the map holds take marks.  n_steps is the sum of those bounds over
 *     the rays that are not skipped, clamped at 0 per ray.  Marks are integers per table slot and do not depend on the
 *     order of the rays: results are deterministic.  They live for one call only, in engine scratch sized by the
 *     capacity; nothing is added to the table's persistent state or to ndt_map_export_state's record.
 *  5. Removal.  A voxel is removed when misses >= min_misses, it took no hit in this call, and protect_min_count == 0
 *     or its count < protect_min_count.  n_voxels_crossed: occupied voxels with at least one miss; n_voxels_hit:
 *     occupied voxels with a hit; n_removed / n_points_removed: the voxels that go and the points they held.
 *     Everything else is ndt_map_crop's contract: when nothing is removed the table is untouched; otherwise the
 *     survivors move bit for bit, moments included, into a fresh table of crop's capacity; ndt_map_get_info reports
 *     the kept voxels and points and their tight ijk box; n_points_dropped, n_adds and n_grows are unchanged; an
 *     emptied map still exists; an allocation failure is NDT_ERR_ALLOC and leaves the map as it was.  With dry_run the
 *     counts are reported and the map is untouched in every case.
 *  6. n == 0 is a no-op with a zeroed result.  No map, a NULL origin or params, a field outside its range or a non-zero
 *     reserved word is NDT_ERR_INVALID_ARG; so are a non-finite pose, an unknown keyframe id and a keyframe form
 *     without a pose.  Nothing changes in any of those cases.  The result pointer may be NULL.  Target, source, align
 *     state, iteration history, evaluation counters and the keyframe archive are left alone, as with ndt_map_crop.
 *     The call is complete when it returns, and the caller's arrays are free. */
typedef struct ndt_map_carve_params {
  int min_misses;        /* >= 1: a voxel goes when at least this many rays of THIS call crossed it */
  int keep_last;         /* >= 0: the last keep_last voxels before a ray's end voxel are never counted (grazing rays) */
  int max_steps;         /* 1 .. 65536: a ray is followed for at most this many voxel steps */
  int protect_min_count; /* 0: off; > 0: a voxel whose count is >= this is never removed */
  int dry_run;           /* != 0: count everything, change nothing */
  int reserved[3];       /* zero */
} ndt_map_carve_params;
typedef struct ndt_map_carve_result {
  int64_t n_rays, n_rays_skipped, n_steps, n_voxels_crossed, n_voxels_hit, n_removed, n_points_removed;
} ndt_map_carve_result;
void ndt_map_carve_default_params(ndt_map_carve_params* p);   /* 2, 1, 4096, 0, 0 */
int ndt_map_carve_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n,
                         const float origin[3], const double* pose16_colmajor_or_null,
                         const ndt_map_carve_params* params, ndt_map_carve_result* out_or_null);
int ndt_map_carve(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, const float origin[3],
                  const double* pose16_colmajor_or_null, const ndt_map_carve_params* params,
                  ndt_map_carve_result* out_or_null);
int ndt_map_carve_keyframe(ndt_handle* h, int64_t id, const float origin[3], const double pose16_colmajor[16],
                           const ndt_map_carve_params* params, ndt_map_carve_result* out_or_null);

/* Connected components of the map: which voxels belong together.  ndt_map_crop removes by position and ndt_map_carve by
 * a later scan's rays; these calls label the occupied voxels by adjacency on the device (a lock-free union-find over the
 * table's slots), report the components, label the points of a cloud by the voxel they fall in, and remove the
 * components a filter rejects: floating speckle, the scraps a carve leaves, the disconnected pieces of a bad merge
 * (pcl::EuclideanClusterExtraction / RadiusOutlierRemoval on a map that keeps no points).  Every output is an integer.
 *  1. Eligible voxels.  An occupied voxel with count >= min_count is eligible; one with count < min_count takes no part:
 *     it joins nothing and bridges nothing.
 *  2. Adjacency.  Two eligible voxels are adjacent when their ijk differ by at most 1 on every axis and the sum s of the
 *     absolute differences is 1 (connectivity 6: faces), 1 <= s <= 2 (18: faces and edges) or 1 <= s <= 3 (26: faces,
 *     edges and corners).
 *  3. No neighbours beyond the range.  A neighbour coordinate with |ijk| >= 2^20 on an axis does not exist (no key is
 *     ever formed from it): (2^20 - 1, 0, 0) and (-(2^20 - 1), 1, 0) are not adjacent.
 *  4. Components.  A component is a class of the transitive closure of adjacency.  Its root is its first voxel in
 *     ascending (k, j, i) order -- ndt_map_export_state's order.
 *  5. Numbering.  Components are numbered 0 .. C - 1 in ascending (k, j, i) order of their roots.  The label of an
 *     eligible voxel is its component's number, the label of an ineligible voxel is -1.
 *  6. Slot independence.  Labels and component records depend on the set of (ijk, count) alone: not on the table's
 *     capacity, not on the order of the adds, not on the slot a voxel sits in.
 * Calls.  Every call takes the params and stands for the map as it is when it is called (the engine may keep a labelling
 * until the map changes; a result after any change of the map is fresh).
 *  - ndt_map_components: labels the map; *info_or_null receives the counts: n_components, the eligible (labelled) and
 *    ineligible (unlabelled) voxels, `largest` = the index of the first component with the most voxels (-1 without one)
 *    and its n_voxels / n_points.  An empty map is NDT_OK with zero components and largest = -1.
 *  - ndt_map_export_components: the C records in index order: root_ijk, n_voxels, n_points (the sum of the voxels'
 *    counts) and the tight ijk box.  Size protocol of ndt_map_export (*n_out = C; at most cap records are written; C > cap
 *    is NDT_ERR_INVALID_ARG behind the write).
 *  - ndt_map_export_labels / _device: every OCCUPIED voxel of the whole map in ndt_map_export_state(NULL, NULL, ...)'s
 *    order -- row r of one is row r of the other -- ijk 3 x int32 and label int32; each may be NULL.  Same size protocol.
 *  - ndt_map_label_points / _device: label_out[p] for the n points of a strided host cloud / SoA device arrays.  A point
 *    is moved by the pose (NULL: none) exactly as ndt_map_add moves it (f64 products summed left to right, one f32
 *    rounding), its voxel is floor(p * inv_leaf) in f32 as for ndt_map_add, its label is that voxel's label; -1 for a
 *    point that is not finite (before or after the pose), beyond the coordinate range, in a voxel the map does not hold
 *    or in an ineligible voxel.  *n_labelled_or_null: the points with a label >= 0.  n == 0 is a no-op (0 labelled).
 *  - ndt_map_remove_components: a component SURVIVES when n_voxels >= min_voxels and n_points >= min_points and
 *    (keep_largest == 0 or its position among ALL components ordered by (n_voxels descending, index ascending) is below
 *    keep_largest).  The eligible voxels of the components that do not survive go; the ineligible voxels go iff
 *    remove_unlabelled != 0.  *out_or_null: n_components, n_components_removed, n_removed (voxels) and
 *    n_points_removed.  Everything else is ndt_map_crop's contract: nothing to remove is NDT_OK with the table untouched;
 *    otherwise the survivors move bit for bit, moments included, into a fresh table of crop's capacity;
 *    ndt_map_get_info reports the kept voxels and points and their tight ijk box; n_points_dropped, n_adds and n_grows
 *    are unchanged; an emptied map still exists; an allocation failure is NDT_ERR_ALLOC and leaves the map as it was.
 *    With dry_run the counts are reported and the map is untouched in every case.
 * Refusals, NDT_ERR_INVALID_ARG with nothing changed: no map; NULL params or filter; a connectivity other than 6, 18, 26;
 * min_count < 1; a non-zero reserved word; min_voxels < 1, min_points < 0 or keep_largest < 0; a non-finite pose; a NULL
 * cloud pointer or a NULL label output with n > 0; a stride below 12 or no multiple of 4; a NULL n_out.  The argument
 * checks come before the handle is looked at.  A bounded loop of the labelling that ran out of its bound is
 * NDT_ERR_INTERNAL (no loop of it waits for another thread).  Target, source, align state, iteration history, evaluation
 * counters and the keyframe archive are left untouched by all calls; the cached levels are left alone except that a
 * removal, as every change of the map, makes them stale.  The calls work on the map itself (also one coarsened by
 * ndt_map_coarsen); components of a cached level or of a box, and clustering the points of a scan without a map, are
 * out of scope.  Complete when they return. */
typedef struct ndt_map_components_params {
  int connectivity;   /* 6 (faces), 18 (faces + edges) or 26 (faces + edges + corners) */
  int min_count;      /* >= 1: a voxel with count < min_count takes no part: it joins nothing and bridges nothing */
  int reserved[2];    /* zero */
} ndt_map_components_params;
typedef struct ndt_map_component {
  int32_t root_ijk[3];                  /* the component's first voxel in ascending (k, j, i) order */
  int32_t n_voxels;
  int64_t n_points;                     /* sum of the voxels' counts */
  int32_t min_ijk[3], max_ijk[3];       /* tight box */
} ndt_map_component;
typedef struct ndt_map_components_info {
  int64_t n_components, n_voxels_labelled, n_voxels_unlabelled;
  int64_t largest;                      /* index of the first component with the most voxels; -1 without one */
  int64_t largest_n_voxels, largest_n_points;
} ndt_map_components_info;
typedef struct ndt_map_component_filter {
  int32_t min_voxels;        /* >= 1 */
  int64_t min_points;        /* >= 0 */
  int32_t keep_largest;      /* 0: off; N > 0: only the N first components in (n_voxels descending, index ascending) order survive */
  int32_t remove_unlabelled; /* != 0: the voxels with count < min_count go as well */
  int32_t dry_run;
  int32_t reserved[3];       /* zero */
} ndt_map_component_filter;
typedef struct ndt_map_remove_components_result {
  int64_t n_components, n_components_removed, n_removed, n_points_removed;
} ndt_map_remove_components_result;
void ndt_map_components_default_params(ndt_map_components_params* p);        /* 26, 1 */
void ndt_map_component_filter_default_params(ndt_map_component_filter* f);   /* 1, 0, 0, 0, 0: removes nothing */
int ndt_map_components(ndt_handle* h, const ndt_map_components_params* params, ndt_map_components_info* info_or_null);
int ndt_map_export_components(ndt_handle* h, const ndt_map_components_params* params, ndt_map_component* comps,
                              size_t cap, size_t* n_out);
int ndt_map_export_labels(ndt_handle* h, const ndt_map_components_params* params, int32_t* ijk, int32_t* label,
                          size_t cap, size_t* n_out);
int ndt_map_export_labels_device(ndt_handle* h, const ndt_map_components_params* params, int32_t* ijk, int32_t* label,
                                 size_t cap, size_t* n_out);
int ndt_map_label_points(ndt_handle* h, const ndt_map_components_params* params, const float* xyz, size_t n,
                         size_t stride_bytes, const double* pose16_colmajor_or_null, int32_t* label_out,
                         int64_t* n_labelled_or_null);
int ndt_map_label_points_device(ndt_handle* h, const ndt_map_components_params* params, const float* dx,
                                const float* dy, const float* dz, size_t n, const double* pose16_colmajor_or_null,
                                int32_t* d_label_out, int64_t* n_labelled_or_null);
int ndt_map_remove_components(ndt_handle* h, const ndt_map_components_params* params,
                              const ndt_map_component_filter* filter, ndt_map_remove_components_result* out_or_null);

/* Re-pose the map: after a pose-graph correction or a loop closure the frame a map was accumulated in moves.  The map
 * has no points to move, but it keeps exactly the sums that move exactly: with p' = R p + t, sum p' and sum p' p'^T are
 * linear in a voxel's count, its three first and its six second moments.  ndt_map_transform moves every voxel of the map
 * by a pose, ndt_map_import_state_posed / _device merge records that were accumulated in another frame (a submap) under
 * the pose that takes that frame to the map's.  Both rest on ONE per-record rule, every operation rounded as written
 * (IEEE f64 unless said otherwise, no contraction):
 *    R_ab = P[a + 4 b], t_a = P[12 + a]: the upper 3 x 4 of the column-major pose AS GIVEN -- there is no orthonormality
 *    check (a scale or a reflection is applied as it stands), and the bottom row is not read beyond the finiteness check,
 *    as with ndt_map_add.  n = (double)count.  lin(a, v) = (R_a0 v0 + R_a1 v1) + R_a2 v2.
 *    float sums  s'_a = (float)(lin(a, (double)s) + n t_a): the one f32 rounding; the intensity sum and the count stay.
 *    moments     u_a = lin(a, m1), m1'_a = u_a + n t_a; with M the symmetric 3 x 3 of {xx, xy, xz, yy, yz, zz}:
 *                A_ab = (R_a0 M_0b + R_a1 M_1b) + R_a2 M_2b, B_ab = (A_a0 R_b0 + A_a1 R_b1) + A_a2 R_b2 for a <= b,
 *                m2'_ab = ((B_ab + u_a t_b) + t_a u_b) + (n t_a) t_b.
 *    voxel       the one ndt_map_add would give a point at the moved FLOAT centroid: c_a = s'_a / (float)count (f32
 *                division), ijk'_a = floor(c_a * inv_leaf) in f32 -- in maps with and without moments alike (the float
 *                centroid is what ndt_map_export shows).  The record's own ijk is not read.
 *    merge       the moved records are merged by ndt_map_import_state's rule: per destination voxel its records in input
 *                order, every field old + record, one rounding.
 * What is exact is the affine map of the sums of one record (up to the roundings written above).  What is not: a moved
 * voxel is assigned as a whole to the voxel of its mean, so points that the new lattice would separate stay together and
 * voxels whose means meet are merged (NDT-OM's map fusion does the same); a moved Gaussian is not split.
 *  - ndt_map_transform: the records are the map's occupied voxels in ascending (k, j, i) order (ndt_map_export_state's
 *    order, so the result does not depend on the table's slot layout); they are merged into a fresh, empty table of the
 *    smallest power-of-two capacity >= 2 x (voxels before) that is not below the capacity ndt_map_reset gave the map, and
 *    the old table is freed only once the new one stands.  Afterwards n_points, n_points_dropped, n_adds and n_grows are
 *    unchanged, n_voxels <= its value before (*n_voxels_after_or_null receives it), min_ijk / max_ijk are the tight box
 *    of the new voxels, the moments and intensity settings are kept.  An empty map is NDT_OK and untouched.  The call
 *    gives up the map's founding property: afterwards ndt_map_export is no longer pcl::VoxelGrid of any concatenation of
 *    clouds.  The identity pose is NOT special-cased: a voxel whose float centroid has rounded out of its own voxel moves
 *    to the voxel the centroid is in.  No record leaves the device.
 *  - ndt_map_import_state_posed / _device: ndt_map_import_state / _device with every record passed through the rule
 *    first (arguments, n = 0, counters, growth and the caller's arrays as there; ijk must not be NULL but is not read).
 * Refusals, each of the whole call with the map exactly as it was, decided before anything is written:
 * NDT_ERR_INVALID_ARG for no map, a NULL pose, a non-finite value in the pose and ndt_map_import_state's own checks
 * (leaf, moments9 on a map with moments, count < 1); NDT_ERR_GRID_OVERFLOW when a moved centroid is not finite or
 * leaves |ijk| < 2^20 (the message names how many); NDT_ERR_ALLOC when an allocation fails.  The target (also one made
 * from this map before), source, align state, iteration history, evaluation counters and the keyframe archive are left
 * untouched.  Complete when they return. */
int ndt_map_transform(ndt_handle* h, const double pose16_colmajor[16], int64_t* n_voxels_after_or_null);
int ndt_map_import_state_posed(ndt_handle* h, float leaf, const int32_t* ijk, const int32_t* count, const float* sums4,
                               const double* moments9, size_t n, const double pose16_colmajor[16]);
int ndt_map_import_state_posed_device(ndt_handle* h, float leaf, const int32_t* ijk, const int32_t* count,
                                      const float* sums4, const double* moments9, size_t n,
                                      const double pose16_colmajor[16]);

/* Levels: the map at leaf * 2^L, made from its own sums, and coarse-to-fine alignment over them.  The points are not
 * kept, but a coarse voxel's sums are the sums of its children's sums, and for a power-of-two factor the parent of a fine
 * voxel is the voxel the point rule gives at the coarse leaf: 1.0f / (leaf * 2^L) is inv_leaf / 2^L exactly and
 * p * (inv_leaf / 2^L) is fl(p * inv_leaf) / 2^L exactly (a division by a power of two does not round a normal f32), so
 * floor(p * inv_leaf_L) == floor_div(floor(p * inv_leaf), 2^L).  A factor that is no power of two has no such identity.
 * THE RULE.  Level L (1 <= L <= NDT_MAP_MAX_LEVEL) of a map with leaf l is a map with leaf_L = (float)(l * 2^L) and
 * inv_leaf_L = 1.0f / leaf_L; a level whose leaf_L is not finite is refused (NDT_ERR_INVALID_ARG).
 *    voxel       every occupied voxel (i, j, k) belongs to the level voxel (i >> L, j >> L, k >> L), an arithmetic shift
 *                (floor_div by 2^L).  That is floor(p * inv_leaf_L) in f32 for every point p of the fine voxel whose
 *                scaled coordinate p * inv_leaf is zero or a normal f32 (a subnormal one, |p| ~ 1e-45, may differ).
 *    count       the sum of the children's counts.  A level voxel whose count would exceed INT32_MAX refuses the level
 *                as a whole (NDT_ERR_GRID_OVERFLOW; nothing is cached, map and target are as they were).
 *    sums        each of the four float sums in f32 and each of the nine moments in f64 starts from +0 and adds the
 *                children's values one at a time in ascending child (k, j, i) order, one rounding per add.  In a map
 *                without intensity the intensity sum is 0; without moments there are no moments.
 * This is ndt_map_import_state of the map's ndt_map_export_state records with ijk shifted, into an empty map of leaf
 * leaf_L, bit for bit.  A level is derived on the device when a call first needs it (no record passes through the host)
 * and cached until the map's content changes (an add, an import, crop, carve, transform, ndt_map_enable_moments);
 * ndt_map_reset, ndt_map_clear and ndt_destroy free the levels.  The level's table has the smallest power-of-two capacity
 * >= 2 x (the map's voxels), at least 64.
 * `level` == 0 is valid in every call below and means the map itself: bit for bit ndt_map_get_info /
 * ndt_map_export_state / _device / ndt_set_target_from_map_moments.  A level outside 0 .. NDT_MAP_MAX_LEVEL is
 * NDT_ERR_INVALID_ARG.  Boxes select level voxels with the level's own inv_leaf_L, as the box rule above reads.
 *  - ndt_map_level_info: derives if stale; leaf, with_intensity, n_voxels, n_points, capacity and the tight min_ijk /
 *    max_ijk are the level's (capacity 0 for a level of an empty map), n_points_dropped, n_adds and n_grows the map's.
 *  - ndt_map_export_state_level / _device: ndt_map_export_state / _device of the level.
 *  - ndt_set_target_from_map_level: ndt_set_target_from_map_moments of the level; ndt_params::resolution must be
 *    bit-equal to leaf_L, and the map must keep moments.
 *  - ndt_map_coarsen: the map BECOMES its level: the level's table replaces the map's, leaf = leaf_L, min_ijk / max_ijk /
 *    n_voxels are the level's, the cached levels are dropped; n_points, n_points_dropped, n_adds, n_grows and the
 *    moments / intensity settings are kept.  Later adds continue as on a map of that leaf.  Level 0 is a no-op.
 *  - ndt_map_levels_drop: frees the cached levels; the map is untouched.
 *  - ndt_align_map_levels (host code): for each of the n_steps (1 .. NDT_MAP_LEVEL_STEPS_MAX) steps in order --
 *    ndt_set_params with resolution = leaf_L of the step's level, the step's max_iterations and step_size (0 / 0.0: the
 *    handle's value); ndt_set_target_from_map_level with the box guess translation +- half_extent (NULL: the whole
 *    level), guess being the previous step's final transform; ndt_align into results[s].  A step that fails stops the call
 *    with its code; earlier results stay written.  On return, success or failure, the handle's ndt_params are the
 *    caller's again, restored through ndt_set_params: THE TARGET IS THE LAST STEP'S TARGET when the caller's resolution
 *    (and the other grid parameters) are that step's, as after a sequence that ends at level 0 of a map whose leaf is
 *    ndt_params::resolution; otherwise ndt_set_params' own rule applies and the target is dropped (no cloud is kept to
 *    re-voxelise).  A NULL pointer or n_steps out of range is NDT_ERR_INVALID_ARG with nothing touched.
 * Every refusal leaves the target and the map as they were.  Source, align state (except through ndt_align_map_levels),
 * iteration history, evaluation counters and the keyframe archive are untouched; only ndt_set_target_from_map_level and
 * ndt_align_map_levels replace the target.  Complete when they return. */
#define NDT_MAP_MAX_LEVEL 6
#define NDT_MAP_LEVEL_STEPS_MAX 8
typedef struct ndt_map_level_step {
  int level;
  int max_iterations;        /* 0: the handle's */
  double step_size;          /* 0.0: the handle's */
} ndt_map_level_step;
int ndt_map_level_info(ndt_handle* h, int level, ndt_map_info* out);
int ndt_map_export_state_level(ndt_handle* h, int level, const float box_min[3], const float box_max[3], int32_t* ijk,
                               int32_t* count, float* sums4, double* moments9, size_t cap, size_t* n_out);
int ndt_map_export_state_level_device(ndt_handle* h, int level, const float box_min[3], const float box_max[3],
                                      int32_t* ijk, int32_t* count, float* sums4, double* moments9, size_t cap,
                                      size_t* n_out);
int ndt_set_target_from_map_level(ndt_handle* h, int level, const float box_min[3], const float box_max[3]);
int ndt_map_coarsen(ndt_handle* h, int level);
int ndt_map_levels_drop(ndt_handle* h);
int ndt_align_map_levels(ndt_handle* h, const ndt_map_level_step* steps, int n_steps, const float half_extent_or_null[3],
                         const float guess_colmajor[16], ndt_result* results);

/* Distribution-to-distribution NDT (D2D; Stoyanov et al. 2012): register a submap's voxels -- Gaussians, not points --
 * to the target's.  It estimates the pose that ndt_map_import_state_posed / ndt_map_transform take, from the two maps'
 * own f64 moments; the chain export -> pose -> posed import runs without a record leaving the device.
 * THE DISTRIBUTION SOURCE is separate from the point source (ndt_set_source*): neither disturbs the other.
 *  - ndt_set_source_distributions / _device take `count` (n) and `moments9` (n x 9: sums of x, y, z, xx, xy, xz, yy, yz,
 *    zz) exactly as ndt_map_export_state / _device write them (host / device memory).  Record r becomes a source Gaussian
 *    when it passes the target build's own leaf rule under the handle's parameters: count >= max(3, min_points_per_voxel),
 *    then the build's finalize step (cov_mode's covariance formula, eigenvalue floor eig_inflation_ratio, the inverse
 *    checks); its mean and its REGULARISED covariance are that leaf's mean and cov as ndt_export_leaves shows them for a
 *    target built from the same moments.  Rejected records are dropped and counted; accepted ones keep input order.
 *    n == 0 clears the source (pointers may be NULL).  NDT_ERR_INVALID_ARG for a NULL pointer with n > 0, a count < 1 or
 *    a non-finite moment: the previous source stays.  The records are kept: when ndt_set_params has changed the leaf rule
 *    the Gaussians are re-derived from them by the next call that uses them.  Complete when they return.
 *  - ndt_source_distributions_info: records handed over and Gaussians accepted (0, 0 without a source).
 *  - ndt_export_source_distributions: the accepted Gaussians -- mean3 (m x 3), cov6 (m x 6: xx, xy, xz, yy, yz, zz), count
 *    and the index of the record each came from (any output may be NULL); returns m, or < 0 (cap < m: INVALID_ARG).
 * THE EVALUATION ndt_eval_derivatives_d2d: K poses p = [x, y, z, roll, pitch, yaw] -> K x NDT_EVAL_WORDS words in the
 * layout of ndt_eval_derivatives (ndt_unpack_eval applies; ridge / regularisation as there).  Per pose, IEEE f64:
 *    rotation    R = Rx(roll) Ry(pitch) Rz(yaw) and its first and second angle derivatives, built on the host from the
 *                sin / cos of poses6 (not from an f32 matrix, no small-angle snap) and handed to the kernel.
 *    moved mean  m_a = ((R_a0 mu_0 + R_a1 mu_1) + R_a2 mu_2) + t_a, rounded as written, no contraction.
 *    neighbours  the target leaves ndt_score_points gives a point at ((float)m_x, (float)m_y, (float)m_z): DIRECT1 or
 *                DIRECT7 by the handle's search method, in the same pair order.
 *    pair (i, j) mu = m - mu_j, C = R Sigma_i R^T + Sigma_j (Sigma_j: the leaf's cov of ndt_export_leaves; of both Sigmas
 *                the triangle xx, xy, xz, yy, yz, zz is what is read), B = C^-1 (by cofactors), q = mu^T B mu, e = exp(-d2 q / 2), score = -d1 e; d1, d2: ndt_gauss_constants of the handle's
 *                resolution and outlier ratio.  A pair whose e is not finite or outside [0, 1] contributes nothing and
 *                is not counted.
 *    gradient    j_a = dm/dp_a, Z_a = (dR/dp_a) Sigma_i R^T + its transpose (0 for translations),
 *                q_a = 2 mu^T B j_a - mu^T B Z_a B mu,  g_a = (d1 d2 / 2) e q_a.
 *    Hessian     H_ab = d2m/dp_a dp_b, Z_ab = (d2R) Sigma_i R^T + (d_a R) Sigma_i (d_b R)^T + transpose,
 *                q_ab = 2 j_b^T B j_a - 2 mu^T B Z_b B j_a + 2 mu^T B H_ab - 2 j_b^T B Z_a B mu + 2 mu^T B Z_b B Z_a B mu
 *                       - mu^T B Z_ab B mu,   Hess_ab = (d1 d2 / 2) e (q_ab - (d2 / 2) q_a q_b):
 *                the exact derivatives of the score (always the full Hessian: hessian_mode is not read).
 *    the rest    nvtl_sum: the sum over Gaussians of their best pair score; n_points_with_neighbors: Gaussians with a
 *                counted pair; n_pairs: counted pairs.  compute_hessian == 0: the Hessian words are zero, score and
 *                gradient are the bits of the Hessian call.
 * Sums are made in a fixed order without float atomics: a call gives the same bits every time, and a pose in a batch of
 * K the bits it gives alone.  NDT_ERR_UNSUPPORTED for NDT_KDTREE / NDT_DIRECT26, a multi-grid union target and a reducer
 * other than NDT_REDUCE_NONE; NDT_ERR_NO_TARGET without a target, NDT_ERR_NO_SOURCE without an accepted Gaussian.
 * THE ALIGN ndt_align_d2d: ndt_newton_align's loop (the ndt_align product path) over that evaluation with the handle's
 * parameters and regularisation pose, n_source_total = the accepted Gaussians; `out` as ndt_align fills it (ms_device 0).
 * Without a target, a distribution source or an accepted Gaussian the guess comes back with converged = 0 and the call
 * returns the code above.  The handle's align state, iteration history, pre-launch state and point source are left alone,
 * as by ndt_align_batch: an ndt_align afterwards gives the bits it gave before. */
int ndt_set_source_distributions(ndt_handle* h, const int32_t* count, const double* moments9, size_t n);
int ndt_set_source_distributions_device(ndt_handle* h, const int32_t* count, const double* moments9, size_t n);
int ndt_source_distributions_info(ndt_handle* h, int64_t* n_records, int64_t* n_accepted);
int64_t ndt_export_source_distributions(ndt_handle* h, double* mean3, double* cov6, int32_t* count, int32_t* record_index,
                                        size_t cap);
int ndt_eval_derivatives_d2d(ndt_handle* h, const double* poses6, int K, int compute_hessian, double* out);
int ndt_align_d2d(ndt_handle* h, const float guess_colmajor[16], ndt_result* out);

/* Continuous-time NDT (CT): align a scan that was captured in motion.  Every other registration call moves the whole
 * scan by one pose; here every point has its own, blended between the scan's known BEGIN pose b (the previous scan's end
 * pose: ndt_result.final_pose of the previous align) and its unknown END pose p = [x, y, z, roll, pitch, yaw] (the pose
 * the drivers attach to a frame) by the point's time factor alpha_i -- one float per point, the reference's pointsAlpha:
 * 0 at the start of the frame, 1 at its end.  ndt_deskew* undoes motion from a trajectory somebody else supplies; here the
 * motion within the scan is part of what the registration estimates.
 * THE TIMES belong to the current point source, in the order the source was handed over.  ndt_set_source_times (host
 * array) / _device (device array, copied; consumed during the call): n must equal ndt_source_size, otherwise
 * NDT_ERR_INVALID_ARG and the previous times stay; n == 0 clears them (the pointer may be NULL).  Values are not checked
 * (see a_i below).  Every call that replaces or re-declares the source drops them: ndt_set_source*, _device,
 * _device_view, ndt_set_source_from_keyframe and ndt_source_changed.  No other call notices the times.
 * ndt_source_times_info: the number of times attached, 0 = none.  Without times (or without a source) the _ct calls
 * return NDT_ERR_NO_SOURCE.  The _ct calls read the source as handed over: source_order is not read, the cached
 * block-ordered copy is neither used nor disturbed.
 * THE EVALUATION ndt_eval_derivatives_ct: K end poses -> K x NDT_EVAL_WORDS words in the layout of ndt_eval_derivatives
 * (ndt_unpack_eval applies; ridge / regularisation as there).  Per pose and point, IEEE f64, no contraction:
 *    a_i         alpha_i clamped to [0, 1].  A point whose alpha or coordinates are not finite contributes nothing and
 *                is not counted.
 *    begin pose  THE FIT, the same in every _ct call: the blend below is linear in the angles, so the begin pose's angles
 *                are first brought onto the Euler branch of the end pose's.  Of the two triples of the begin rotation
 *                -- (r, p, y) as given and (r + pi, pi - p, y + pi) -- each angle is shifted by round((angle - end's
 *                angle) / 2 pi) turns (nothing is subtracted for 0 turns), and the triple whose three absolute
 *                differences to the end pose's angles then add up to less is taken (a tie keeps the first).  A begin
 *                pose already on the branch is used bit for bit; the translation is never touched.  b below is the
 *                fitted begin pose.  This is what lets the previous result's final_pose be handed in as it is: those
 *                angles come out of ndt_newton_align's matrix-to-pose conversion, which folds the roll into [0, pi], so
 *                a roll that changes sign between two scans -- or a yaw that crosses pi -- puts two consecutive results
 *                on different triples of nearly the same rotation.
 *    pose        p_i = b + a_i (p - b), component by component, rounded as written; a_i == 1 uses p itself, a_i == 0 uses
 *                b itself.  The end pose's angles are used as given.
 *    moved point R_i = Rx(roll) Ry(pitch) Rz(yaw) of p_i's angles (the convention of ndt_eval_derivatives_d2d), sin and
 *                cos per point in f64, applied one rotation after the other, every operation rounded as written:
 *                  u = (cy x0 - sy x1, sy x0 + cy x1, x2)        v = (cp u0 + sp u2, u1, cp u2 - sp u0)
 *                  w = (v0, cr v1 - sr v2, sr v1 + cr v2)        x'_i = w + t_i
 *    neighbours  the target leaves ndt_score_points gives a point at ((float)x', (float)y', (float)z'): DIRECT1 or
 *                DIRECT7 by the handle's search method, in the same pair order.
 *    pair (i, j) mu = x'_i - mean_j, B = the leaf's icov as ndt_export_leaves shows it (its triangle xx, xy, xz, yy, yz,
 *                zz is what is read), q = mu^T B mu, e = exp(-d2 q / 2); a pair whose e is not finite or outside [0, 1]
 *                contributes nothing and is not counted; score += -d1 e; d1, d2: ndt_gauss_constants of the handle's
 *                resolution and outlier ratio.
 *    derivatives with j_c = d x'_i / d (p_i)_c (a unit vector for a translation, (dR/d angle_c) x_i for a rotation) and
 *                h_cd its second derivative (non-zero for rotation pairs only), and because d p_i / d p = a_i I:
 *                  g_c  += a_i d1 d2 e (mu^T B j_c)
 *                  H_cd += a_i^2 d1 d2 e ( -d2 (mu^T B j_c)(mu^T B j_d) + mu^T B h_cd + j_d^T B j_c )
 *                the exact gradient and Hessian of the score (always the full Hessian: hessian_mode is not read).
 *    the rest    nvtl_sum, n_points_with_neighbors and n_pairs as in ndt_eval_derivatives.  compute_hessian == 0: the
 *                Hessian words are zero, score and gradient are the bits of the Hessian call.
 * With every alpha_i = 1 this is the ordinary point-to-distribution evaluation at p, in f64.  With b == p every point
 * lands where that evaluation puts it, so score, nvtl_sum and the counters do not depend on the times; gradient and
 * Hessian still do -- they are derivatives with respect to the END pose, of which point i follows the share a_i, so they
 * are the a_i- and a_i^2-weighted sums of that evaluation's per-point terms.  Sums are made in a fixed order without float atomics: a call gives the same bits
 * every time, and a pose in a batch of K the bits it gives alone.
 * NDT_ERR_INVALID_ARG, before the handle is looked at, for a NULL pointer, K <= 0 or a non-finite pose entry;
 * NDT_ERR_UNSUPPORTED for NDT_KDTREE / NDT_DIRECT26, a multi-grid union target and a reducer other than
 * NDT_REDUCE_NONE; NDT_ERR_NO_TARGET as for ndt_align; NDT_ERR_NO_SOURCE without a source or without times.
 * THE ALIGN ndt_align_ct: ndt_newton_align's loop (the ndt_align product path: the Hessian in every trial, the memo on)
 * over that evaluation with the handle's parameters and regularisation pose, n_source_total = the source size; `out` as
 * ndt_align fills it (ms_device 0), final_pose being the END pose.  The begin pose is fitted ONCE, before the loop, to
 * the guess's pose -- the one ndt_newton_align derives from the matrix, on whose branch final_pose then lies -- and not
 * again per evaluation, so the objective does not change under the loop.  On a failure before the loop `out` holds the
 * guess with converged = 0.  The handle's align state, iteration history, pre-launch state and evaluation counters are left alone:
 * an ndt_align afterwards gives the bits it gave before.
 * THE DESKEWED SCAN ndt_transform_source_ct (host output, n x 3 floats) / _device (three device arrays): the source
 * under begin pose b (fitted to e as above: a begin pose and a result on different Euler triples deskew as the align
 * saw them) and end pose e, out[i] belonging to in[i].
 *    frame == 1  the points in the target's frame: y = x'_i as above.
 *    frame == 0  the points in the END pose's frame -- what goes into ndt_keyframe_put or ndt_map_add with the result:
 *                y = R(e)^T (x'_i - t(e)), the three rotations of e undone one after the other (Rx^T, Ry^T, Rz^T).  A
 *                point whose pose p_i equals e in all six numbers (a_i == 1, or b == e) comes back bit for bit: "no
 *                motion" is exact, as in ndt_deskew.
 * Everything is computed in f64 and rounded to f32 once.  A non-finite point or time gives NaN in x, y and z.
 * cap < n is NDT_ERR_INVALID_ARG and nothing is written; frame other than 0 / 1 and a non-finite pose entry likewise.
 * The blend is linear in the Euler parameters, not a slerp: exact for a constant-rate yaw, second-order different from
 * ndt_deskew's trajectory model otherwise. */
int     ndt_set_source_times(ndt_handle* h, const float* alpha, size_t n);
int     ndt_set_source_times_device(ndt_handle* h, const float* d_alpha, size_t n);
int64_t ndt_source_times_info(const ndt_handle* h);
int     ndt_eval_derivatives_ct(ndt_handle* h, const double begin_pose6[6], const double* poses6, int K,
                                int compute_hessian, double* out);
int     ndt_align_ct(ndt_handle* h, const double begin_pose6[6], const float guess_colmajor[16], ndt_result* out);
int     ndt_transform_source_ct(ndt_handle* h, const double begin_pose6[6], const double end_pose6[6], int frame,
                                float* out_xyz, size_t cap_points);
int     ndt_transform_source_ct_device(ndt_handle* h, const double begin_pose6[6], const double end_pose6[6], int frame,
                                       float* ox, float* oy, float* oz, size_t cap);

/* Generalised ICP (GICP; Segal, Haehnel & Thrun, RSS 2009) in the plane-to-plane form of PCL / pclomp: the third method of
 * the registration boundary beside NDT and SVN-NDT, and a cross-check of an NDT result -- same clouds, no voxel grid.  It
 * registers the current POINT source (ndt_set_source*) to the points the target was built from (a target that keeps no
 * points -- ndt_set_target_device*, a multi-grid union -- is NDT_ERR_UNSUPPORTED, as for ndt_fitness_score).  Everything
 * below is IEEE arithmetic rounded as written, no contraction; tests/test_gicp_cpu.py restates it in NumPy.
 * PARAMETERS ndt_gicp_params (defaults: ndt_gicp_default_params): k_neighbours 20 (PCL's correspondence randomness; 4 ..
 * 32), max_neighbour_distance +INF (> 0; finite: bounds the neighbour search of isolated points), covariance_epsilon 1e-3
 * (PCL's gicp_epsilon; in (0, 1]), max_correspondence_distance D = 5.0 (> 0, +INF allowed), transformation_epsilon 1e-4
 * (finite, >= 0), max_iterations 64 (outer loop, >= 1), max_inner_iterations 20 (>= 1).  ndt_gicp_set_params: a NULL
 * pointer or a value outside these ranges (NaN included) is NDT_ERR_INVALID_ARG before the handle is looked at, and
 * nothing changes.  A changed k_neighbours, max_neighbour_distance or covariance_epsilon drops the cached covariances of
 * both clouds (and the pairs); a changed max_correspondence_distance drops the pairs.
 * NEIGHBOURS of point i of a cloud (`which`: NDT_GICP_SOURCE or NDT_GICP_TARGET), a point being FINITE when x, y and z are:
 *    d2(i, j) = (dx*dx + dy*dy) + dz*dz in f32, dx = x_j - x_i and so on, rounded as written.
 *    The neighbours are the m <= k finite points j of the SAME cloud with the smallest (d2, j) in lexicographic order, i
 *    itself included (d2 = 0), restricted to d2 <= (float)(cap * cap) when max_neighbour_distance = cap is finite.  The
 *    search is exact: it does not depend on how the engine indexes the cloud.  A point that is not finite has m = 0.
 *    A point with m < 4 HAS NO COVARIANCE: it takes no part in anything below and is counted.
 * COVARIANCE of a point with m >= 4, f64, over its neighbour list in that order (x_j: the f32 coordinates as f64):
 *    mean_a   = (sum over the list in order, starting from 0) / m
 *    raw_ab   = (sum over the list in order of (x_ja - mean_a) * (x_jb - mean_b), starting from 0) / m, ab over xx, xy,
 *               xz, yy, yz, zz
 *    n        = the unit eigenvector of the smallest eigenvalue of raw, by the target build's cyclic Jacobi in f64
 *               (columns sorted by ascending eigenvalue; numpy.linalg.eigh agrees to a few ulp where the two smallest
 *               eigenvalues are apart)
 *    C_ab     = delta_ab - ((1 - eps) * n_a) * n_b, eps = covariance_epsilon: PCL's U diag(1, 1, eps) U^T, written so that
 *               it depends on the normal alone (xy, xz, yz are computed once: C is symmetric bit for bit).
 * The lists and covariances are derived lazily by the first call that needs them and cached: the source's until a call
 * replaces or re-declares the source (ndt_set_source*, _device, _device_view, ndt_set_source_from_keyframe,
 * ndt_source_changed), the target's until the target changes.
 *  - ndt_gicp_export_neighbours: idx (n x k_neighbours int32, row i in (d2, j) order, -1 padded) and n_found (n int32), rows
 *    in input order; either may be NULL.  Returns n, or < 0 (cap < n: NDT_ERR_INVALID_ARG).
 *  - ndt_gicp_export_covariances: mean3 (n x 3), raw_cov6 (n x 6), cov6 (n x 6), rows in input order, NaN rows for points
 *    without a covariance; any may be NULL.  Returns n, or < 0.
 * PAIRING ndt_gicp_pair(pose6 = [x, y, z, roll, pitch, yaw]): for every source point with a covariance
 *    rotation    R = Rx(roll) Ry(pitch) Rz(yaw), built on the host in f64 from the sin / cos of pose6, as for
 *                ndt_eval_derivatives_d2d.
 *    moved point x'_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a in f64 (that rule's moved mean), query = its f32 rounding.
 *    partner     the finite target point j with the smallest (d2, j), d2 = (dx*dx + dy*dy) + dz*dz in f32 between the
 *                query and the target point (target - query), found exactly.  It is kept when d2 <= (float)(D * D),
 *                inclusive, and when j has a covariance.
 *    Otherwise -- and for a source point without a covariance or a query that is not finite -- the entry is -1 with d2 = +INF.
 * The pairs are FROZEN in the handle until the next pairing, a source or target change, or a parameter change.
 * *n_pairs (nullable): the kept pairs.  ndt_gicp_export_pairs: target_index (n int32) and d2 (n floats) in source order,
 * either may be NULL; returns n, 0 without frozen pairs, or < 0.
 * THE EVALUATION ndt_eval_derivatives_gicp: K poses -> K x NDT_EVAL_WORDS words in the layout of ndt_eval_derivatives
 * (ndt_unpack_eval applies; ridge / regularisation as there) over the FROZEN pairs, IEEE f64.  Per pair (i, j), with the
 * rotation and moved point of the pairing at the evaluated pose:
 *    mu = x'_i - b_j (b_j: the target point), C = R C_i R^T + C_j, B = C^-1 (by cofactors), q = mu^T B mu;
 *    score += -q / 2, gradient_a += -q_a / 2, Hessian_ab += -q_ab / 2, q_a and q_ab EXACTLY the expressions of
 *    ndt_eval_derivatives_d2d with Sigma_i = C_i, Sigma_j = C_j (the same device function with the weight f = -1/2 in
 *    place of (d1 d2 / 2) e, and without the (d2 / 2) q_a q_b term).  A pair whose q is not finite contributes nothing
 *    and is not counted.  nvtl_sum = score; n_points_with_neighbors = n_pairs = the counted pairs.
 * compute_hessian == 0: the Hessian words are zero, score and gradient are the bits of the Hessian call.  Sums are made in
 * a fixed order without float atomics: the same bits every time, and a pose in a batch of K gets the bits it gets alone.
 * NDT_ERR_INVALID_ARG, before the handle is looked at, for a NULL pointer, K <= 0 or a non-finite pose entry;
 * NDT_ERR_UNSUPPORTED with a reducer other than NDT_REDUCE_NONE and for a target that keeps no points; NDT_ERR_NO_TARGET
 * without a target; NDT_ERR_NO_SOURCE without a source or without frozen pairs.
 * THE ALIGN ndt_align_gicp, PCL's two-level loop.  p_0 = the pose ndt_newton_align derives from the guess matrix, T_0 = the
 * guess.  Outer iteration s = 0 .. max_iterations - 1:
 *    1. ndt_gicp_pair at p_s; zero pairs end the call with NDT_ERR_NO_SOURCE.
 *    2. ndt_newton_align's loop (the ndt_align product path) from T_s over the evaluation above, with the handle's
 *       ndt_params except trans_epsilon = transformation_epsilon and max_iterations = max_inner_iterations, n_source_total
 *       = the source size: result r_s.  p_{s+1} = r_s.final_pose, T_{s+1} = r_s.final_transformation.
 *    3. stop, converged, when sqrt(sum_c (p_{s+1,c} - p_{s,c})^2) < transformation_epsilon -- the criterion that loop
 *       applies to the length of a step.  After max_iterations outer iterations the call ends with converged = 0.
 * `out` is the last inner result as ndt_align_d2d fills it, with converged as above, iterations = the outer iterations,
 * n_evaluations / n_evaluations_reused summed over the inner loops and ms_total the whole call.  `info` (nullable): outer
 * iterations, inner iterations summed, evaluations summed, the pairs of the last pairing, the points without a covariance
 * of either cloud.  On every failure `out` holds the guess with converged = 0.  The handle's align state, iteration history,
 * pre-launch state, point source and distribution source are left alone, as by ndt_align_d2d: an ndt_align afterwards gives
 * the bits it gave before, and so do the fitness calls (they share the target's point index). */
#define NDT_GICP_SOURCE 0
#define NDT_GICP_TARGET 1
typedef struct ndt_gicp_params {
  int k_neighbours;
  double max_neighbour_distance;
  double covariance_epsilon;
  double max_correspondence_distance;
  double transformation_epsilon;
  int max_iterations;
  int max_inner_iterations;
} ndt_gicp_params;
typedef struct ndt_gicp_info {
  int outer_iterations;
  int inner_iterations;
  int n_evaluations;
  int64_t n_pairs;
  int64_t n_source_without_covariance;
  int64_t n_target_without_covariance;
} ndt_gicp_info;
void    ndt_gicp_default_params(ndt_gicp_params* p);
int     ndt_gicp_set_params(ndt_handle* h, const ndt_gicp_params* p);
int     ndt_gicp_get_params(const ndt_handle* h, ndt_gicp_params* p);
int64_t ndt_gicp_export_neighbours(ndt_handle* h, int which, int32_t* idx, int32_t* n_found, size_t cap);
int64_t ndt_gicp_export_covariances(ndt_handle* h, int which, double* mean3, double* raw_cov6, double* cov6, size_t cap);
int     ndt_gicp_pair(ndt_handle* h, const double pose6[6], int64_t* n_pairs);
int64_t ndt_gicp_export_pairs(ndt_handle* h, int32_t* target_index, float* d2, size_t cap);
int     ndt_eval_derivatives_gicp(ndt_handle* h, const double* poses6, int K, int compute_hessian, double* out);
int     ndt_align_gicp(ndt_handle* h, const float guess_colmajor[16], ndt_result* out, ndt_gicp_info* info);

/* Voxelised GICP (VGICP; Koide, Yokozuka, Oishi & Banno, ICRA 2021): GICP's plane-to-plane cost with ONE AGGREGATE PER
 * TARGET VOXEL as the partner of a source point -- the mean of the voxel's points and the mean of their GICP covariances,
 * found by a voxel lookup.  There is no nearest-point search at evaluation time, there are no frozen pairs and there is no
 * outer re-pairing loop: the align is one Newton loop, as for NDT.  The point covariances of both clouds are GICP's, under
 * the handle's ndt_gicp_params (of which only k_neighbours, max_neighbour_distance and covariance_epsilon are read here).
 * Everything below is IEEE arithmetic rounded as written, no contraction; tests/test_vgicp_cpu.py restates it in NumPy.
 * VOXELS.  A VGICP voxel is a leaf of the built NDT target: one row per leaf in the order of ndt_export_leaves.  The
 * handle's resolution, min_points_per_voxel and leaf rule (eigenvalue checks included) decide which voxels exist: a caller
 * who wants sparse voxels lowers min_points_per_voxel, whose floor is 3.  Target point j CONTRIBUTES to leaf l when it is
 * finite, has a covariance (m >= 4 neighbours under the GICP rule above) and the f32 classification of the target build --
 * in = lo <= p < hi per axis, i_a = (int)(floorf(p_a * inv_leaf) - (float)min_b_a), the classification ndt_score_points
 * gives the unmoved point -- puts it into the cell of leaf l.  The aggregates, f64, over the contributing points in
 * ascending input index:
 *    N_l      = their number
 *    mean_a   = (sum of (double)x_ja, starting from 0) / N_l
 *    cov_ab   = (sum of C_j,ab, starting from 0) / N_l, ab over xx, xy, xz, yy, yz, zz; C_j: the regularised covariance
 *               ndt_gicp_export_covariances shows
 * A leaf with N_l = 0 has NaN rows and never pairs.  The sums are made in a fixed order without float atomics.  The table
 * is derived lazily by the first call that needs it and cached; it is dropped when the target changes, when
 * ndt_set_params rebuilds the grid and when ndt_gicp_set_params changes k_neighbours, max_neighbour_distance or
 * covariance_epsilon.
 *  - ndt_vgicp_export_voxels: count (n_leaves int32), mean3 (n_leaves x 3), cov6 (n_leaves x 6); any may be NULL.  Returns
 *    n_leaves, or < 0 (cap < n_leaves: NDT_ERR_INVALID_ARG).
 *  - ndt_vgicp_get_info: derives the table if needed (and the source's covariances when a source is set); the pair fields
 *    are 0.
 * THE EVALUATION ndt_eval_derivatives_vgicp: K poses -> K x NDT_EVAL_WORDS words in the layout of ndt_eval_derivatives
 * (ndt_unpack_eval applies; ridge / regularisation as there), IEEE f64.  Per source point i with a covariance:
 *    rotation, moved point x' and its f32 query: exactly those of ndt_gicp_pair / ndt_eval_derivatives_d2d.
 *    partners    the leaves ndt_score_points gives a point at that query: DIRECT1 or DIRECT7 by the handle's search
 *                method, in the same pair order.
 *    pair (i, l) with N_l >= 1: mu = x' - mean_l, C = R C_i R^T + cov_l, B = C^-1 (by cofactors), q = mu^T B mu,
 *                f = -0.5 * (double)N_l; score += f * q, gradient_a += f * q_a, Hessian_ab += f * q_ab, q_a and q_ab
 *                EXACTLY the expressions of ndt_eval_derivatives_d2d (the same device function), without the q_a q_b
 *                term.  A pair whose q is not finite contributes nothing and is not counted.
 *    nvtl_sum = score; n_points_with_neighbors = the source points with a counted pair; n_pairs = the counted pairs.
 * compute_hessian == 0: the Hessian words are zero, score and gradient are the bits of the Hessian call.  The same bits
 * every time, and a pose in a batch of K gets the bits it gets alone.
 * DIRECT7 is the wider and the LESS EXACT neighbourhood: the cost is quadratic (no exponential cuts a far partner off),
 * so the neighbouring voxels of other surfaces pull on a point.  It pairs almost every source point and tolerates a
 * worse guess; DIRECT1 ends closer to the true pose (DESIGN 7q has the figures).
 * NDT_ERR_INVALID_ARG, before the handle is looked at, for a NULL pointer, K <= 0 or a non-finite pose entry;
 * NDT_ERR_UNSUPPORTED for a target that keeps no points (ndt_set_target_device*), a multi-grid union, NDT_KDTREE /
 * NDT_DIRECT26 and a reducer other than NDT_REDUCE_NONE; NDT_ERR_NO_TARGET without a target; NDT_ERR_NO_SOURCE without a
 * source or without a source point that has a covariance.
 * THE ALIGN ndt_align_vgicp: ONE run of ndt_newton_align's loop (the ndt_align product path) over that evaluation with the
 * handle's ndt_params and regularisation pose, n_source_total = the source size; `out` as ndt_align_d2d fills it.  There is
 * no outer loop.  `info` (nullable): the table's counters, the points without a covariance of either cloud, and the pairs
 * of the last evaluation of the loop.  On every failure `out` holds the guess with converged = 0.  The handle's align
 * state, iteration history, pre-launch state, point source, distribution source and frozen GICP pairs are left alone: an
 * ndt_align, an ndt_align_gicp and the fitness calls afterwards give the bits they gave before. */
typedef struct ndt_vgicp_info {
  int64_t n_voxels;                    /* leaves with N_l >= 1 */
  int64_t n_leaves;                    /* rows of the table */
  int64_t n_target_points_in_voxels;   /* sum of N_l */
  int64_t n_target_without_covariance;
  int64_t n_source_without_covariance;
  int64_t n_pairs, n_source_with_pairs;   /* of the last evaluation of the align */
} ndt_vgicp_info;
int64_t ndt_vgicp_export_voxels(ndt_handle* h, int32_t* count, double* mean3, double* cov6, size_t cap);
int     ndt_vgicp_get_info(ndt_handle* h, ndt_vgicp_info* out);
int     ndt_eval_derivatives_vgicp(ndt_handle* h, const double* poses6, int K, int compute_hessian, double* out);
int     ndt_align_vgicp(ndt_handle* h, const float guess_colmajor[16], ndt_result* out, ndt_vgicp_info* info_or_null);

/* Scan Context place recognition (Kim & Kim, IROS 2018) over the device keyframe archive: which archived scan shows this
 * place again, and under which heading -- the question in front of ndt_align_batch / ndt_align_d2d (the relative pose) and
 * ndt_map_transform / ndt_map_import_state_posed (the correction).  A scan becomes an n_rings x n_sectors matrix of
 * maximum heights around the sensor; two matrices are compared by the mean cosine distance of their columns, minimised
 * over ALL cyclic column shifts, against EVERY descriptor of the bank in one launch (no ring key, no k-d tree).  The best
 * shift is the relative yaw.  Everything below is IEEE arithmetic rounded as written, no contraction; the results equal a
 * NumPy restatement bit for bit (tests/test_scan_context_cpu.py).
 * PARAMETERS (R = n_rings, S = n_sectors): 1 <= R <= 32, 3 <= S <= 128, max_radius finite and > 0, z_sign exactly +1 or
 * -1, lift finite, min_points_per_bin >= 1; anything else is NDT_ERR_INVALID_ARG and the previous state stays.  Defaults:
 * 20, 60, 80.0f, +1.0f, 2.0f, 1.  ndt_scan_context_set_params with a CHANGE clears the descriptor bank (its entries were
 * made under other parameters); the same parameters again change nothing.
 * THE DESCRIPTOR RULE
 *    sector table  dir[k] = ((float)cos(2 pi k / S), (float)sin(2 pi k / S)), cosine and sine computed by the host in f64
 *                  and rounded to f32 once.  ndt_scan_context_sector_table (host only, S x 2 floats) returns it and the
 *                  engine uploads this very table.
 *    a point       (x, y, z) in f32 is SKIPPED when a coordinate is not finite, when x == 0 && y == 0, or when it fails
 *                  the ring gate below.
 *    sector        c_k = (double)dir[k].x * (double)y - (double)dir[k].y * (double)x; both products are exact in f64, so
 *                  the sign of c_k is exact.  The sector is the one s with c_s >= 0 and c_{(s+1) mod S} < 0 (for S >= 3
 *                  it exists and is unique off the origin).  The kernel guesses s with atan2f and settles it with these
 *                  tests.
 *    ring          r2 = (double)x * (double)x + (double)y * (double)y, rho = sqrt(r2); the point is skipped unless
 *                  rho < (double)max_radius; ring = min((int)(rho * (double)R / (double)max_radius), R - 1).
 *    height        hgt = z_sign * z + lift in f32 (the product is exact: one rounding).
 *    bin (ring, s) count = the unskipped points of the bin (int32); desc = the maximum over them of max(hgt, +0.0f), and
 *                  +0.0f when count < min_points_per_bin.
 *    layout        desc[ring * S + s], count likewise.
 * Maximum and integer sum do not depend on order: the kernel's integer atomics (on the bit pattern of the non-negative
 * floats, and on the counts) are deterministic, and the host, device and keyframe forms give the same bits.  n == 0 gives
 * the all-zero descriptor.
 * THE MATCH RULE (Q the query, C a bank entry, both R x S f32; all arithmetic f64)
 *    nQ[j] = sqrt(sum_r (double)Q[r][j]^2), r ascending, one rounding per addition; nC likewise.
 *    for each shift n = 0 .. S-1: sum = 0, m = 0; for j = 0 .. S-1 ascending, jj = (j + n) mod S: the column is skipped
 *    when nQ[j] == 0 or nC[jj] == 0, otherwise dot = sum_r (double)Q[r][j] * (double)C[r][jj] (r ascending),
 *    sum += 1.0 - dot / (nQ[j] * nC[jj]), m += 1;  d(n) = m > 0 ? sum / m : 1.0.
 *    distance = min_n d(n) (d(0) first, then every d(n) < the best so far), shift = the smallest n that attains it,
 *    columns = that shift's m.
 * yaw = shift * 2 pi / S wrapped to (-pi, pi]; Rz(yaw) about the frame's own z axis is the guess for aligning the QUERY
 * scan (source) to the CANDIDATE scan (target): a sensor yawed by +psi sees the world at azimuth alpha - psi, so
 * Q[:, j] ~ C[:, j + psi S / 2 pi].  Fixed order, no float atomics: an entry matched in a bank of 10 000 has the bits it has
 * when matched alone.
 * THE CALLS.  A NULL handle or a NULL required pointer is NDT_ERR_INVALID_ARG before the handle is read.  Every call is
 * complete when it returns and is ordered on the handle's stream like the other blocking calls.
 *  - ndt_scan_context (host cloud, xyz + stride as ndt_set_source) / _device (three device arrays; d_desc, d_count device
 *    memory of R x S words) / _keyframe (the archived scan `id`; the descriptor goes into the bank under the same id,
 *    replacing an entry, and optionally to the host): desc R x S floats, count R x S int32 (may be NULL).  An unknown
 *    keyframe id is NDT_ERR_INVALID_ARG.
 *  - the bank: _bank_put stores a saved descriptor under `id` (replacing), _bank_get reads one back, _bank_erase drops one,
 *    _bank_clear all, _bank_count counts; an unknown id in get / erase is NDT_ERR_INVALID_ARG.  ndt_keyframe_erase does not
 *    touch the bank.
 *  - ndt_scan_context_match (query from the host) / _match_keyframe (query = bank entry `id`, read on the device; its own
 *    entry is among the results; an unknown id is NDT_ERR_INVALID_ARG): return m, the number of bank entries, and fill ids,
 *    distance, shift, columns (each may be NULL) for all m entries in ascending id order; cap < m is NDT_ERR_INVALID_ARG;
 *    an empty bank returns 0. */
typedef struct { int32_t n_rings, n_sectors; float max_radius, z_sign, lift; int32_t min_points_per_bin; } ndt_scan_context_params;
void    ndt_scan_context_default_params(ndt_scan_context_params* p);
int     ndt_scan_context_set_params(ndt_handle* h, const ndt_scan_context_params* p);
int     ndt_scan_context_get_params(const ndt_handle* h, ndt_scan_context_params* p);
int     ndt_scan_context_sector_table(int n_sectors, float* dir_xy);
int     ndt_scan_context(ndt_handle* h, const float* xyz, size_t n, size_t stride_bytes, float* desc, int32_t* count_or_null);
int     ndt_scan_context_device(ndt_handle* h, const float* dx, const float* dy, const float* dz, size_t n, float* d_desc, int32_t* d_count_or_null);
int     ndt_scan_context_keyframe(ndt_handle* h, int64_t id, float* desc_or_null, int32_t* count_or_null);
int     ndt_scan_context_bank_put(ndt_handle* h, int64_t id, const float* desc);
int     ndt_scan_context_bank_get(ndt_handle* h, int64_t id, float* desc);
int     ndt_scan_context_bank_erase(ndt_handle* h, int64_t id);
int     ndt_scan_context_bank_clear(ndt_handle* h);
int64_t ndt_scan_context_bank_count(const ndt_handle* h);
int64_t ndt_scan_context_match(ndt_handle* h, const float* desc, int64_t* ids, double* distance, int32_t* shift, int32_t* columns, size_t cap);
int64_t ndt_scan_context_match_keyframe(ndt_handle* h, int64_t id, int64_t* ids, double* distance, int32_t* shift, int32_t* columns, size_t cap);

/* setRegularizationPose (ref: run/pipeline_ligo_tc.cpp:531) */
int ndt_set_regularization_pose(ndt_handle* h, const float pose_colmajor[16]);
int ndt_clear_regularization_pose(ndt_handle* h);

/* ---- registration ------------------------------------------------------- */
/* align(out, guess) / computeTransformation (ref: run/pipeline.cpp:561,
 * test_svn_ndt.cpp:171).  Blocks until the result is on the host. */
int ndt_align(ndt_handle* h, const float guess_colmajor[16], ndt_result* out);

/* pclomp::NdtResult's per-iteration arrays [RECALLED: tier4 ndt_omp's transformation_array,
 * transform_probability_array, nearest_voxel_transformation_likelihood_array; the reference's drivers read none of them]
 * of the LAST ndt_align on this handle: entry 0 is the initial guess with the scores of the first evaluation, then one
 * entry per Newton iteration (the transform after it, the scores of its accepted evaluation).  Any output may be NULL;
 * at most `cap` entries are written; returns the number of entries available (iterations + 1) or < 0. */
int ndt_get_iteration_history(const ndt_handle* h, float* transforms16_colmajor, double* transform_probability,
                              double* nearest_voxel_transformation_likelihood, int cap);

/* Derivatives at K poses in one call (computeDerivatives; and Stage 1 of
 * svn_ndt::align, ref: svn_ndt_impl.hpp:758-781).  poses6: K x 6 doubles.
 * transforms: optional K x 16 floats (column-major) applied to the source;
 * NULL = the matrix built from each pose.  out: K x NDT_EVAL_WORDS doubles. */
int ndt_eval_derivatives(ndt_handle* h, const double* poses6, const float* transforms,
                         int K, int compute_hessian, double* out);
/* unpack one evaluation into score, g[6], H[36] (row-major) */
void ndt_unpack_eval(const double* eval_words, double* score, double* g6, double* H36);
/* The two pose-only ingredients of an evaluation as the engine computes them on the host, no handle and no device
 * needed (round 5; the C++ adapter builds the reference's public per-pair math hooks on them):
 * - the angular tables of computeAngleDerivatives for pose [x, y, z, roll, pitch, yaw] (ref: svn_ndt_impl.hpp:254-331):
 *   j_ang as 8 rows x 3 floats, h_ang as 15 rows x 3 floats -- the words every k_derivatives launch receives;
 * - the Gaussian constants d1, d2 of updateNdtConstants (ref: svn_ndt_impl.hpp:90-130). */
int ndt_angle_tables(const double pose6[6], float j_ang[24], float h_ang[45]);
int ndt_gauss_constants(double resolution, double outlier_ratio, double* d1, double* d2);

/* Scoring-only evaluation (pclomp's calculateTransformationProbability /
 * calculateNearestVoxelTransformationLikelihood [RECALLED]; the reference names them only through
 * SURVEY 8f-4): score, transform probability (score / #source points) and NVTL (mean over the points
 * that have a neighbour of their best per-voxel score) of the current source under T against the
 * current target.  One launch of the score-only kernel: no gradient, no Hessian. */
typedef struct ndt_score {
  double score;
  double transform_probability;
  double nearest_voxel_transformation_likelihood;
  int64_t n_pairs;
  int64_t n_points_with_neighbors;
} ndt_score;
int ndt_score_transform(ndt_handle* h, const float T_colmajor[16], ndt_score* out);
/* K transforms (K x 16 floats) scored in ONE launch of the batched score-only kernel */
int ndt_score_transforms(ndt_handle* h, const float* transforms_colmajor, int K, ndt_score* out);

/* 2-D (x, y) covariance estimators of tier4 ndt_omp's estimate_covariance.cpp.
 * [RECALLED]: the file is in the un-vendored submodule; the reference names it only in its build
 * (ref: CMakeLists.txt:40) and no driver calls it.  cov_xy: 2x2 row-major.
 *  - Laplace approximation: -(H[0:2,0:2])^-1 of a result's Hessian;
 *  - poses to search: (offset_x, offset_y) pairs rotated onto the principal axes of that
 *    covariance and added to the result's translation (n x 16 floats out);
 *  - MULTI_NDT: re-align from every pose, unbiased sample covariance of the (x, y) of the main
 *    result and the n re-aligned results (the handle's last result is the last re-alignment);
 *  - MULTI_NDT_SCORE: NVTL of the source at every pose -- one batched launch --, weights
 *    softmax(NVTL / temperature) over {main result} + poses, weighted mean and covariance. */
int ndt_xy_covariance_laplace(const double hessian36[36], double cov_xy[4]);
int ndt_propose_poses_to_search(const ndt_result* r, const double* offsets_x, const double* offsets_y, int n,
                                float* poses16_out);
int ndt_xy_covariance_multi_ndt(ndt_handle* h, const ndt_result* main_result, const float* poses16, int n,
                                double mean_xy[2], double cov_xy[4]);
int ndt_xy_covariance_multi_ndt_score(ndt_handle* h, const ndt_result* main_result, const float* poses16, int n,
                                      double temperature, double mean_xy[2], double cov_xy[4]);

/* Covariance of a registration result for the pose graph: cov = -(H + eps I)^-1 of
 * ndt_result.hessian (ref: run/pipeline.cpp:594-596, eps = 1e-6 there), and with
 * gtsam_order != 0 the block permutation of RegisterCallback::reorderCovarianceForGTSAM
 * (ref: src/registercallback.cpp:170-186: rotation block first, cross blocks left where
 * they are).  Host-only, no handle.  NDT_ERR_INVALID_ARG when H + eps I is singular or
 * not finite. */
int ndt_result_covariance(const double hessian36[36], double eps, int gtsam_order, double cov36[36]);

/* output cloud of align(): source transformed by T (device-side), packed xyz */
int ndt_transform_source(ndt_handle* h, const float T_colmajor[16], float* out_xyz, size_t cap_points);

/* getFitnessScore(max_range) [RECALLED: PCL 1.14 Registration::getFitnessScore, registration.hpp]: every source point
 * is moved by T (the f32 arithmetic of ndt_transform_source, bit for bit), its squared distance d^2 to the NEAREST RAW
 * target point is found (exactly: a point-level index over the target's points, not the voxel grid), and the mean of
 * d^2 over the points with d^2 <= max_range (squared distance, inclusive) is the fitness.  Deviations: non-finite target
 * points are not candidates; non-finite source points are skipped (neither counted nor summed).  The index is built
 * by the first fitness call after the target changed and kept until the next ndt_set_target*, keyframe target or
 * resolution-driven rebuild; targets consumed through ndt_set_target_device* (nothing retained) and multi-grid targets
 * are NDT_ERR_UNSUPPORTED.  With a sharded source the result covers the local shard: ranks add sum_sq_dist and
 * n_inliers themselves.  Results are bit-reproducible (fixed-order f64 sums, no float atomics). */
typedef struct ndt_fitness {
  double fitness_score;   /* sum_sq_dist / n_inliers, DBL_MAX when n_inliers == 0 */
  double sum_sq_dist;     /* f64 sum of d^2 over the inliers */
  int64_t n_inliers;      /* finite source points with d^2 <= max_range */
  int64_t n_points;       /* finite source points queried */
} ndt_fitness;
/* sq_dists_out (nullable, host, cap >= n_source): per source point d^2 to its nearest target point;
 * NaN for a non-finite source point, +INF where d^2 > max_range (not searched exactly) */
int ndt_fitness_score(ndt_handle* h, const float T_colmajor[16], double max_range, ndt_fitness* out,
                      float* sq_dists_out, size_t cap);
/* K transforms (K x 16 floats, column-major) in one query launch; out[k] equals ndt_fitness_score at transform k */
int ndt_fitness_scores(ndt_handle* h, const float* transforms_colmajor, int K, double max_range, ndt_fitness* out);

/* Per-point view of a scoring-only evaluation [RECALLED: tier4 ndt_omp's calculateNearestVoxelScoreEachPoint]: what
 * ndt_score_transform adds up, kept per source point, in the order the source was handed over (whatever
 * ndt_source_order says; viewed and keyframe sources included).  The point is moved by T with the f32 arithmetic of an
 * evaluation, so it has exactly the neighbour voxels it has there.  Per point:
 *   score                sum over its neighbour voxels of the pair score -d1 * exp(-d2/2 * q), the evaluation's guards
 *   nearest_voxel_score  its largest pair score; 0 without a neighbour
 *   n_neighbors          its (point, voxel) pairs, as counted for ndt_score.n_pairs
 *   best_voxel           ndt_leaf.index of the voxel that gave nearest_voxel_score (multi-grid union: the cell's index);
 *                        -1 without a contributing pair, i.e. exactly where nearest_voxel_score == 0; on equal scores
 *                        the smallest index
 * A source point that is not finite, or not finite after the transform, reports 0 / 0 / 0 / -1.  Hence, in either
 * record format: sum(score) = ndt_score.score, sum(n_neighbors) = n_pairs, count(n_neighbors > 0) =
 * n_points_with_neighbors, mean of nearest_voxel_score over those = NVTL (up to the order of the f64 additions).
 * Any output may be NULL; cap >= n_source for those that are not (NDT_ERR_INVALID_ARG).  One plain launch on the
 * engine's stream; a pending deferred build is settled first and the errors are those of ndt_score_transform.  The align
 * state, the iteration history and the evaluation counters of the handle are left alone.  A sharded source reports its
 * local shard. */
int ndt_score_points(ndt_handle* h, const float T_colmajor[16], double* score, double* nearest_voxel_score,
                     int32_t* n_neighbors, int64_t* best_voxel, size_t cap);
/* the same into caller-owned DEVICE arrays; complete when the call returns */
int ndt_score_points_device(ndt_handle* h, const float T_colmajor[16], double* d_score, double* d_nearest_voxel_score,
                            int32_t* d_n_neighbors, int64_t* d_best_voxel, size_t cap);
/* number of points of the current (local) source: the n_source the calls above size their outputs by; < 0 on error */
int64_t ndt_source_size(const ndt_handle* h);

/* Score-based filter of the source on the device.  Writes the source points (as handed over, NOT transformed) whose
 * nearest_voxel_score under T is >= min_score (keep_below != 0: those below it, points without a neighbour included)
 * to device SoA arrays, in input order -- the selection is exactly that comparison applied to what ndt_score_points
 * returns for the same T.  At most cap points are written.  *n_out is the number selected.  NDT_ERR_INVALID_ARG if it
 * exceeds cap (cap = n_source always suffices), or if min_score is NaN.  d_index_out (nullable) receives each selected
 * point's position in the source.  Complete when the call returns: the arrays can go straight into
 * ndt_set_target_device or ndt_set_source_device.  The handle's own source is unchanged.  Stable and deterministic:
 * wave ballots, block scans and integer block offsets, no atomics. */
int ndt_filter_source_device(ndt_handle* h, const float T_colmajor[16], double min_score, int keep_below,
                             float* ox, float* oy, float* oz, int32_t* d_index_out, size_t cap, size_t* n_out);
/* packed xyz and indices in host memory */
int ndt_filter_source(ndt_handle* h, const float T_colmajor[16], double min_score, int keep_below,
                      float* out_xyz, int32_t* index_out, size_t cap_points, size_t* n_out);

/* ---- voxel grid accessors ------------------------------------------------ */
int ndt_get_grid_info(const ndt_handle* h, ndt_grid_info* out);
/* getTargetCells().getLeaves(): valid leaves sorted by ascending index; returns
 * the number written (<= cap) or < 0 */
int64_t ndt_export_leaves(ndt_handle* h, ndt_leaf* out, size_t cap);

/* ---- host Newton driver with an external evaluator ----------------------- */
/* fn must fill out[NDT_EVAL_WORDS] with the GLOBAL (already reduced) evaluation
 * at pose6 / T; return 0 on success. */
typedef int (*ndt_eval_fn)(void* ctx, const double pose6[6], const float T_colmajor[16],
                           int compute_hessian, double out[NDT_EVAL_WORDS]);
int ndt_newton_align(const ndt_params* p, int64_t n_source_total,
                     const float guess_colmajor[16], const float* regularization_pose_or_null,
                     ndt_eval_fn fn, void* ctx, ndt_result* out);

/* ---- multi-hypothesis align: K Newton loops in lockstep, one batched evaluation per round ---- */
#define NDT_ALIGN_BATCH_MAX 256
/* Host-only counterpart of ndt_newton_align for K guesses (K x 16 floats, column-major), 1 <= K <= NDT_ALIGN_BATCH_MAX.
 * In every round each hypothesis still running advances on the host until it needs an evaluation or stops; fn then
 * receives the requests of those K_round hypotheses, in hypothesis order (poses6: K_round x 6, T16: K_round x 16
 * column-major, need_h: K_round flags), and fills out[K_round x NDT_EVAL_WORDS] with the GLOBAL evaluations.  Each
 * hypothesis behaves as ndt_newton_align from its guess with the same evaluator (trials without the Hessian, one
 * re-evaluation at the accepted step, no memo), so out[k] is what ndt_newton_align gives for guess k; ms_total is the
 * wall time of the whole call.  A failing fn ends the call with its code.  NDT_ERR_INVALID_ARG for K outside the range
 * or a NULL pointer (regularization_pose_or_null excepted). */
typedef int (*ndt_eval_batch_fn)(void* ctx, int K, const double* poses6, const float* T16, const int* need_h,
                                 double* out);
int ndt_newton_align_batch(const ndt_params* p, int64_t n_source_total, const float* guesses16_colmajor, int K,
                           const float* regularization_pose_or_null, ndt_eval_batch_fn fn, void* ctx, ndt_result* out);
/* align(guess_k) for k < K against the handle's target, source, parameters and regularisation pose: K Newton /
 * More-Thuente loops of the ndt_align product path (the Hessian in every trial, repeated requests answered without a
 * launch) advanced in lockstep, the pending evaluations of one round in ONE batched kernel launch -- so a call costs
 * max_k n_evaluations launches (ndt_timing.n_eval_launches), not their sum.
 *  - arguments: 1 <= K <= NDT_ALIGN_BATCH_MAX and no NULL pointer, else NDT_ERR_INVALID_ARG (out untouched);
 *  - out[k] is filled as ndt_align fills its result; n_evaluations / n_evaluations_reused are per hypothesis, ms_total
 *    is the wall time of the call, ms_device the device time of its launches while kernel timing is on;
 *  - without a target (or after a failed deferred build) every out[k] holds its guess with converged = 0, and the call
 *    returns what ndt_align would; a reducer other than NDT_REDUCE_NONE is NDT_ERR_UNSUPPORTED (guesses in out);
 *  - the handle's align state is left alone: ndt_get_iteration_history still reports the last ndt_align, the
 *    pre-launch and stream-placement state is not touched, and an ndt_align after the call gives the bits it gave before;
 *  - independence: out[k] depends on guess k alone -- not on the other guesses, their order or how many are still
 *    running in a round -- as long as the source is evaluated in the order it was handed over (NDT_SOURCE_ORDER_KEEP, or
 *    AUTO below its sort threshold).  A source the engine sorts is sorted once per (source, target), by the guess of
 *    the first call that needs it (here guesses[0]), and every round of the call keeps that order;
 *  - where the single-pose and batched launches partition the source alike (at most 512 points per compute unit:
 *    131 072 on an MI355X), out[k] is bit-identical to ndt_align(guess k) but for the timings. */
int ndt_align_batch(ndt_handle* h, const float* guesses16_colmajor, int K, ndt_result* out);

/* ---- multi-GPU: one process per GPU, source sharded, target replicated ---- */
/* contiguous shard of n items for rank r of nranks */
void ndt_shard_range(size_t n, int rank, int nranks, size_t* begin, size_t* count);
/* rank 0 creates the id (128 bytes) and the caller broadcasts it (e.g. through
 * torch.distributed); then every rank calls ndt_comm_init_rccl. */
int ndt_comm_unique_id(void* out128);
int ndt_comm_init_rccl(ndt_handle* h, const void* id128, int rank, int nranks);
/* host-side reduction through a POSIX shared-memory segment named `name` */
int ndt_comm_init_shm(ndt_handle* h, const char* name, int rank, int nranks);
/* Peer-write reducer (NDT_REDUCE_P2P).  Every rank calls ndt_comm_p2p_handle (allocates its exchange
 * area in fine-grained device memory on the handle's device and exports it as an IPC handle of
 * NDT_P2P_HANDLE_BYTES), the caller all-gathers the handles (bench.py: over its shared-memory board), then
 * every rank calls ndt_comm_init_p2p with all of them in rank order.  Ranks are processes; all their
 * devices must be visible to each other (no HIP_VISIBLE_DEVICES masking per rank). */
#define NDT_P2P_HANDLE_BYTES 64
int ndt_comm_p2p_handle(ndt_handle* h, void* out_handle);
int ndt_comm_init_p2p(ndt_handle* h, const void* handles, int rank, int nranks);
/* First-contact instrumentation of the peer-write reducer (round 5).
 * ndt_comm_p2p_selftest: COLLECTIVE (every rank, same `rounds`; put a barrier of your own behind it): `rounds` lock-step rounds
 * of patterned {tag, value} slots through the exchange areas, written and read exactly as the derivative kernel's final sum
 * does it -- the direct test of "a 16-byte slot is seen entirely old or entirely new" across devices.  out: {rounds completed,
 * slots seen with a new tag and an old value, rounds a peer missed (the pass stops at the first), longest round in 10 ns ticks}.
 * ndt_comm_p2p_stats: out = {exchanges made inside a kernel's final sum since ndt_comm_init_p2p (or the last reset), their
 * summed duration and the longest one in 10 ns ticks (own row published -> every rank's row read), exchanges a peer was late for}. */
int ndt_comm_p2p_selftest(ndt_handle* h, int rounds, int64_t out[4]);
int ndt_comm_p2p_stats(ndt_handle* h, int64_t out[4], int reset);
/* caller-supplied all-reduce(sum) over NDT_EVAL_WORDS doubles, in place */
typedef int (*ndt_allreduce_fn)(void* ctx, double* words, int n);
int ndt_comm_init_hook(ndt_handle* h, ndt_allreduce_fn fn, void* ctx, int rank, int nranks);
int ndt_comm_destroy(ndt_handle* h);
/* which collective library serves the RCCL reducer: ncclGetVersion() code (e.g. 22105) and the
 * path of the shared object the symbol was resolved from (the process may hold two librccl.so:
 * ROCm's and the one bundled with PyTorch); returns the version or < 0 */
int ndt_comm_info(char* path_buf, size_t cap);
/* ranks of the handle's live reducer as the transport reports them (RCCL: ncclCommCount of the engine's
 * communicator); 1 without a reducer; < 0 on failure */
int ndt_comm_rank_count(const ndt_handle* h);
/* total source points over all ranks (for transform_probability); set by the
 * caller after sharding, defaults to the local count */
int ndt_set_global_source_size(ndt_handle* h, int64_t n_total);

/* ---- SVN-NDT (svn_ndt::SvnNormalDistributionsTransform::align) ------------- */
/* Stein Variational Newton over K pose particles (ref: extern/svn_ndt/include/svn_ndt.h:
 * 100-182, svn_ndt_impl.hpp:675-964; driver: run/pipeline_lo_svn.cpp:301-319,387-388).
 * Stage 1 (NDT derivatives of every particle) is one batched kernel launch; stages 2-3
 * run on the host.  The engine's ndt_params select the svn defaults through
 * hessian_mode = NDT_HESSIAN_GAUSS_NEWTON and add_ridge = 1 (svn_ndt.h:314,
 * svn_ndt_impl.hpp:650-653).  Poses are 4x4 double, column-major; covariance 6x6 row-major
 * in GTSAM tangent order [rot, trans] (svn_ndt.h:46). */
typedef struct ndt_svn_params {
  int particle_count;      /* setParticleCount (30) */
  int max_iterations;      /* setMaxIterations (50) */
  double kernel_bandwidth; /* setKernelBandwidth (1.0) */
  double step_size;        /* setStepSize (1.0) */
  double stop_threshold;   /* setEarlyStopThreshold (1e-4) */
} ndt_svn_params;

typedef struct ndt_svn_result {  /* svn_ndt::SvnNdtResult (svn_ndt.h:40-51) */
  double final_pose[16];
  double final_covariance[36];
  int converged;
  int iterations;
  double last_mean_update;   /* |Log(mean_prev^-1 mean)| of the last iteration */
  double ms_total, ms_stage1, ms_stage2, ms_stage3;
} ndt_svn_result;

void ndt_svn_default_params(ndt_svn_params* p);
/* prior.retract(sigma * N(0,1)) for K particles (ref :708-716); the reference seeds from the
 * wall clock, here the seed is explicit.  particles16: K x 16 doubles. */
int ndt_svn_sample_particles(const double prior16[16], int K, uint64_t seed, double* particles16);
/* The particle kernel of Stage 2 for ONE pair, as ndt_svn_align evaluates it (round 5; host arithmetic, no handle):
 * k = exp(-|Log(l^-1 k)|^2 / bandwidth) and, if grad6 != NULL, its gradient with respect to l in l's tangent space,
 * [rotation, translation] (ref: rbf_kernel / rbf_kernel_gradient, svn_ndt_impl.hpp:213-244).  Poses: 4 x 4 column-major. */
int ndt_svn_rbf_kernel(const double pose_l16[16], const double pose_k16[16], double bandwidth, double* k, double* grad6);
/* particles16 (K x 16): initial particles in, final particles out.  The source / target
 * clouds are those of the handle (ndt_set_target / ndt_set_source). */
int ndt_svn_align(ndt_handle* h, const ndt_svn_params* p, const double prior16[16],
                  double* particles16, ndt_svn_result* out);

/* ---- instrumentation ------------------------------------------------------ */
typedef struct ndt_timing {
  double ms_last_eval_kernel;   /* HIP-event time of the last derivative kernel */
  double ms_last_reduce_kernel; /* round 5: wall time of the last CROSS-RANK sum on the host (shm / hook transports; 0 without
                                 * a reducer; the peer-write exchange runs inside the kernel: ndt_comm_p2p_stats) */
  double ms_last_build;         /* the last target build: HIP-event time of its launches while kernel timing is on, else wall time
                                 * from its enqueue to its verdict.  ndt_set_target_from_map_moments and the multi-grid union
                                 * always report the wall time of the whole call, its host waits included (so does
                                 * ndt_grid_info::ms_build) */
  int64_t n_eval_launches;      /* since handle creation */
  double ms_eval_kernel_total;  /* summed HIP-event time of the accumulation kernel while timing is on */
  double ms_reduce_kernel_total;
  int64_t n_timed_evals;        /* evaluations covered by the two totals */
} ndt_timing;
int ndt_enable_kernel_timing(ndt_handle* h, int on);
int ndt_get_timing(const ndt_handle* h, ndt_timing* out);

/* Breakdown of the last host hand-off of each cloud (ndt_set_target* / ndt_set_source* from host memory). */
typedef struct ndt_handoff_lane_timing {
  int64_t n_points;
  int64_t bytes_in;     /* bytes of the caller's cloud that were read (n x stride, or 12 n for SoA) */
  int64_t bytes_dma;    /* bytes that crossed PCIe (12 n) */
  double ms_repack;     /* host time of the call up to its return in asynchronous mode: wait for the staging buffer,
                           AoS -> chunk-major repack on `threads` threads, issue of the copies and the SoA kernel */
  double ms_dma;        /* device time from before the first copy to behind the last, by HIP events; only while kernel
                           timing is enabled (ndt_enable_kernel_timing) and once the hand-off has completed */
  double dma_gb_per_s;  /* bytes_dma / ms_dma */
  int threads;          /* repack threads incl. the caller */
} ndt_handoff_lane_timing;
typedef struct ndt_handoff_timing {
  ndt_handoff_lane_timing target, source;
  double ms_build_wait; /* time the first call that needed the grid waited for the deferred build's verdict */
  int mode;             /* ndt_handoff_mode */
  int cpu_budget;       /* CPUs this process may use (affinity mask cut down to the cgroup quota) */
  int repack_workers;   /* worker threads of the repack pool (NDT_UPLOAD_THREADS overrides) */
} ndt_handoff_timing;
int ndt_get_handoff_timing(const ndt_handle* h, ndt_handoff_timing* out);

#ifdef __cplusplus
}
#endif
#endif /* NDT_HIP_H_ */
