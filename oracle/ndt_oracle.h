/*
 * ndt_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU float64 restatement of the reference's NDT scan-matching path
 * (khalisfadil/slam-sam). It exists to CHECK the HIP product path; nothing
 * under slam-sam_amd/ or include/ may link, import or call it.  Allowed
 * callers: tests/, __graft_entry__.smoke(), bench.py's cpu_baseline leg.
 *
 * PARITY STATUS: pinned only at the level of the reference's single test for
 * this path (extern/svn_ndt/test/test_svn_ndt.cpp:138-199,
 * ConvergenceComparison.PclOmp: converged, < 50 iterations, <= 0.05 m and
 * <= 0.035 rad from ground truth on the two-plane fixture :44-83).  The
 * reference holds no golden vectors for score / gradient / Hessian / leaves,
 * and its ndt_omp submodule is absent, so DERIVATIVE-LEVEL PARITY IS UNPINNED.
 *
 * Reference files restated (all under /root/reference, cited per function):
 *   extern/svn_ndt/include/voxel_grid_covariance_impl.hpp   voxel grid + lookups
 *   extern/svn_ndt/include/voxel_grid_covariance.h          Leaf, defaults, getLeaf
 *   extern/svn_ndt/include/svn_ndt_impl.hpp                 NDT constants + derivatives
 * The Newton / More-Thuente loop lives in the un-vendored tier4/ndt_omp
 * submodule (extern/ndt_omp is empty; pinned revision unknown) and is restated
 * from the published algorithm (Magnusson 2009 Alg. 2; More & Thuente 1994;
 * Sun & Yuan 2006 eq. 2.4.2/2.4.5/2.4.52/2.4.56), anchored on the reference's
 * call sites run/pipeline.cpp:464-481,557-568 and test_svn_ndt.cpp:144-179.
 */
#ifndef NDT_ORACLE_H_
#define NDT_ORACLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { ORACLE_DIRECT1 = 1, ORACLE_DIRECT7 = 7, ORACLE_DIRECT26 = 26, ORACLE_KDTREE = 27 };
enum { ORACLE_HESSIAN_FULL = 0, ORACLE_HESSIAN_GAUSS_NEWTON = 1 };
/* covariance normalisation: vendored svn code uses /n then *n/(n-1)
 * (voxel_grid_covariance_impl.hpp:287-291); upstream PCL/pclomp is recalled
 * to use the "(n-1)/n" form -- unverifiable here, kept as a switch. */
enum { ORACLE_COV_SVN = 0, ORACLE_COV_PCL_RECALLED = 1 };
/* per-pair arithmetic: vendored (f64 Mahalanobis + exp, guards 50 / 1e-15,
 * svn_ndt_impl.hpp:418-447; products of the gradient / Hessian terms in f32, :412-415,
 * :449-494) or upstream pclomp as recalled (all-f32, [0,1] guard).
 * ORACLE_PAIR_SVN_F64: the vendored FORMULAS with every product carried in f64 -- not what
 * the reference computes, but what its f32 products approximate; lets the tests separate
 * "the kernel implements other formulas" (never) from "the reference rounds to f32"
 * (1e-7 per product, up to ~4e-5 of the sums on ill-conditioned voxels). */
enum { ORACLE_PAIR_SVN = 0, ORACLE_PAIR_PCLOMP_RECALLED = 1, ORACLE_PAIR_SVN_F64 = 2 };

typedef struct oracle_params {
  float resolution;            /* voxel leaf size (m) */
  double outlier_ratio;        /* svn_ndt.h:287 default 0.55 */
  double step_size;            /* More-Thuente step_max */
  double trans_epsilon;        /* convergence threshold on step length */
  int max_iterations;
  int search_method;           /* ORACLE_DIRECT1 / ORACLE_DIRECT7 / ORACLE_DIRECT26 [RECALLED] / ORACLE_KDTREE */
  int min_points_per_voxel;    /* voxel_grid_covariance.h:153 default 6 */
  double eig_inflation_ratio;  /* voxel_grid_covariance.h:154 default 0.01 */
  int hessian_mode;            /* full analytic (pclomp) or Gauss-Newton (svn default) */
  int cov_mode;
  int pair_mode;
  int add_ridge;               /* H += 1e-6 I (svn_ndt_impl.hpp:650-653) */
  int use_line_search;         /* 1 = More-Thuente, 0 = fixed step min(|dp|, step_size) */
  int num_threads;             /* OpenMP threads for the per-point loop */
  int use_regularization;      /* tier4 longitudinal regularisation [RECALLED] */
  float regularization_scale_factor;
  float regularization_pose[16]; /* column-major 4x4 */
  int symmetrize_hessian;      /* test seam: mirror the upper triangle of H (the f32 J^T C^-1 J
                                  product of svn_ndt_impl.hpp:470 is only symmetric to rounding) */
} oracle_params;

void oracle_default_params(oracle_params* p);

typedef struct oracle_grid oracle_grid;

typedef struct oracle_grid_info {
  int min_b[3], max_b[3], div_b[3];
  float leaf, inv_leaf;
  int64_t n_leaves;     /* valid leaves kept */
  int64_t n_cells_hit;  /* cells with >= 1 point before filtering */
} oracle_grid_info;

/* xyz: n points, stride_bytes between consecutive points (12 packed, 32 PCL AoS) */
oracle_grid* oracle_grid_build(const float* xyz, size_t n, size_t stride_bytes,
                               const oracle_params* prm);
void oracle_grid_free(oracle_grid* g);
void oracle_grid_get_info(const oracle_grid* g, oracle_grid_info* out);
/* leaves are exported sorted by ascending 1-D cell index */
void oracle_grid_export(const oracle_grid* g, int64_t* cell, int32_t* count,
                        double* mean3, double* cov9, double* icov9,
                        double* evecs9, double* evals3);
/* neighbourhood of one point: writes up to 27 leaf ranks (index into the exported order),
 * returns the count.  ORACLE_KDTREE = radius search (radius = leaf size) over the f32
 * centroids of the valid leaves (ref: voxel_grid_covariance_impl.hpp:505-554, centroids
 * :386-435, radius svn_ndt_impl.hpp:579): a centroid within one leaf size of the point can
 * only sit in the 3x3x3 cells around it, so those 27 cells are scanned instead of a kd-tree;
 * FLANN's test `dist^2 < radius^2` in f32 is kept. */
int oracle_grid_neighbors(const oracle_grid* g, const float p[3], int method,
                          int64_t out_rank[27]);

/* Gauss constants (svn_ndt_impl.hpp:80-131): out = {d1, d2, d3} */
void oracle_gauss_constants(double resolution, double outlier_ratio, double out[3]);

/* angle tables (svn_ndt_impl.hpp:255-334): j_ang 8x3, h_ang 15x3 (f32 values widened) */
void oracle_angle_tables(const double pose6[6], float j_ang[24], float h_ang[45]);

/* 4x4 f32 transform (column-major) from p=[x,y,z,roll,pitch,yaw], R=Rx*Ry*Rz */
void oracle_pose_to_matrix(const double pose6[6], float T[16]);
/* inverse mapping with Eigen's eulerAngles(0,1,2) convention */
void oracle_matrix_to_pose(const float T[16], double pose6[6]);

typedef struct oracle_derivs {
  double score;
  double gradient[6];
  double hessian[36];       /* row-major (symmetric) */
  double nvtl_sum;          /* sum over points of the best per-pair score */
  int64_t n_with_neighbors; /* points with >= 1 valid neighbour voxel */
  int64_t n_pairs;          /* total (point, voxel) pairs visited */
} oracle_derivs;

/* svn_ndt_impl.hpp:518-668 (per-cloud accumulation). T (column-major f32 4x4) is
 * the transform applied to the source; pose6 feeds the angle tables. */
void oracle_derivatives(const oracle_grid* g, const float* src_xyz, size_t n,
                        size_t stride_bytes, const float T[16], const double pose6[6],
                        const oracle_params* prm, int compute_hessian,
                        oracle_derivs* out);

typedef struct oracle_result {
  float final_transformation[16]; /* column-major */
  double final_pose[6];
  int converged;
  int iterations;
  int n_evaluations;
  double hessian[36];
  double score;
  double transform_probability;
  double nvtl;
  /* trajectory log, up to 128 iterations */
  int n_logged;
  double log_pose[128][6];
  double log_step[128];
  double log_score[128];
} oracle_result;

/* Newton + More-Thuente (pclomp computeTransformation, restated) */
void oracle_align(const oracle_grid* g, const float* src_xyz, size_t n,
                  size_t stride_bytes, const float guess[16],
                  const oracle_params* prm, oracle_result* out);

/* The reference test fixture (test_svn_ndt.cpp:44-83,104-111): two planes,
 * 134*134*2 = 35912 pts; target = gt(source) + N(0, sigma) from
 * std::default_random_engine(1337).  Returns the point count; buffers must hold
 * 3*35912 floats each.  gt16/guess16 column-major f64. */
size_t oracle_two_plane_fixture(float* src_xyz, float* tgt_xyz, double gt16[16],
                                double guess16[16]);

/* ---- SVN-NDT outer loop (ref: extern/svn_ndt/include/svn_ndt_impl.hpp:675-964) ----------
 * Stein Variational Newton over K pose particles; Stage 1 = oracle_derivatives per particle
 * (Gauss-Newton Hessian + 1e-6 ridge by default, svn_ndt.h:314), Stage 2 = RBF-kernel mix and
 * a 6x6 solve per particle in GTSAM tangent order [rot, trans], Stage 3 = retraction.  GTSAM's
 * Pose3 Expmap / Logmap / between / rpy are restated from their published formulas; retract is
 * taken as the full exponential map (GTSAM_POSE3_EXPMAP, the default since GTSAM 4.1).
 * The reference seeds its particle sampler from the wall clock (:712); here the initial
 * particles are an input so runs are reproducible. */
typedef struct oracle_svn_params {
  int particle_count;      /* K_ (svn_ndt.h default 30) */
  int max_iterations;      /* max_iter_ (50) */
  double kernel_bandwidth; /* kernel_h_ (1.0) */
  double step_size;        /* step_size_ (1.0) */
  double stop_threshold;   /* stop_thresh_ (1e-4) */
} oracle_svn_params;

typedef struct oracle_svn_result {
  double final_pose[16];        /* column-major 4x4 */
  double final_covariance[36];  /* row-major, GTSAM order [rot, trans] */
  int converged;
  int iterations;
  int n_logged;                 /* iterations logged below (<= 128) */
  double log_mean_update[128];  /* |Log(mean_prev^-1 mean_cur)| per iteration */
} oracle_svn_result;

/* particles: K x 16 doubles (column-major poses), updated in place to the final particles */
void oracle_svn_align(const oracle_grid* g, const float* src_xyz, size_t n, size_t stride_bytes,
                      const double prior16[16], double* particles, const oracle_params* prm,
                      const oracle_svn_params* svn, oracle_svn_result* out);
/* prior.retract(sigma .* N(0,1)) for K particles with sigmas (0.01,0.01,0.02,0.05,0.05,0.05)
 * in GTSAM order (ref :708-716), std::mt19937_64(seed) + std::normal_distribution */
void oracle_svn_sample_particles(const double prior16[16], int K, uint64_t seed, double* particles);
/* SE(3) helpers exported for tests: xi = [omega, v] (GTSAM order) */
void oracle_se3_expmap(const double xi[6], double T16[16]);
// Limit of the logarithm (gtsam's formulas, restated as they are): the generic branch divides by 2 sin(theta), so its
// error grows as 1e-16 pi / sin(theta)^2 (1e-9 at pi - 1e-3); where trace + 1 < 1e-10 (within 1e-5 rad of pi) it
// returns the angle pi itself and an axis whose sign is fixed by convention, not by R - R^T: off by pi - theta, and
// by the sign for half of the axes.  Nothing the SVN loop feeds it comes near pi (particle pairs are centimetres and
// milliradians apart); tests/test_attitudes_cpu.py pins the size of the limit.
void oracle_se3_logmap(const double T16[16], double xi[6]);

#ifdef __cplusplus
}
#endif
#endif
