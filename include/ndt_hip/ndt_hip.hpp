// ndt_hip.hpp -- header-only C++ adapter over the C-ABI (include/ndt_hip.h) with the method
// names AND the value types of `pclomp::NormalDistributionsTransform` /
// `svn_ndt::SvnNormalDistributionsTransform` that the reference's drivers use
// (ref: run/pipeline.cpp:464-481,557-604; run/pipeline_ligo_tc.cpp:287-305,529-541;
//  run/pipeline_ins_map_distribution.cpp:346-371; run/pipeline_lo_svn.cpp:299-320,387-388;
//  include/pipeline.hpp:163-222; extern/svn_ndt/test/test_svn_ndt.cpp:144-179).
//
// Three optional faces, detected with __has_include (or forced with -DNDT_HIP_WITH_*=0/1):
//   * Eigen  (<Eigen/Core>): Matrix4f / Matrix6d / Vector3d / Matrix3d ARE the Eigen types, so
//     `ndt_result.hessian + Matrix6d::Identity() * 1e-6` (run/pipeline.cpp:594-596) and
//     `.mean = leaf.getMean()` (include/pipeline.hpp:196-201) compile as written.
//     Without Eigen they are small column-major POD matrices with the same accessors.
//   * PCL    (<pcl/registration/registration.h>, needs Eigen): the engine derives from
//     `pcl::Registration`, so it can be stored in `RegisterCallback::registration`
//     (ref: include/registercallback.hpp:35) and driven through setInputTarget /
//     setInputSource / align / getFinalTransformation / hasConverged.
//   * GTSAM  (<gtsam/geometry/Pose3.h>): `SvnNormalDistributionsTransform::align(cloud,
//     gtsam::Pose3)` returning `SvnNdtResult{gtsam::Pose3 final_pose; Matrix6d
//     final_covariance; ...}` (ref: extern/svn_ndt/include/svn_ndt.h:40-51,100-182).
// include/compat/ holds `pclomp/ndt_omp.h`, `svn_ndt.h`, ... that alias the reference's
// namespaces onto this header: with that directory in front of extern/ndt_omp/include and
// extern/svn_ndt/include the drivers compile unchanged.
//
// The build image has neither Eigen, PCL nor GTSAM: the three faces are compile- and run-tested
// against minimal API mocks (tests/cpp/mock/, test doubles -- not the libraries), the plain face
// by tests/cpp/test_adapter.cpp.
//
// Failures never throw: like the reference (ref: svn_ndt_impl.hpp:682-702) a failed align
// leaves the guess as the final transformation and hasConverged() == false; the status and
// message are available through lastStatus() / lastError().
#pragma once

#include <algorithm>
#include <cmath>
#include <array>
#include <cstddef>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../ndt_hip.h"

#if !defined(NDT_HIP_WITH_EIGEN)
#if defined(__has_include)
#if __has_include(<Eigen/Core>)
#define NDT_HIP_WITH_EIGEN 1
#endif
#endif
#endif
#ifndef NDT_HIP_WITH_EIGEN
#define NDT_HIP_WITH_EIGEN 0
#endif

#if !defined(NDT_HIP_WITH_PCL)
#if NDT_HIP_WITH_EIGEN && defined(__has_include)
#if __has_include(<pcl/registration/registration.h>)
#define NDT_HIP_WITH_PCL 1
#endif
#endif
#endif
#ifndef NDT_HIP_WITH_PCL
#define NDT_HIP_WITH_PCL 0
#endif

#if !defined(NDT_HIP_WITH_GTSAM)
#if NDT_HIP_WITH_EIGEN && defined(__has_include)
#if __has_include(<gtsam/geometry/Pose3.h>)
#define NDT_HIP_WITH_GTSAM 1
#endif
#endif
#endif
#ifndef NDT_HIP_WITH_GTSAM
#define NDT_HIP_WITH_GTSAM 0
#endif

#if NDT_HIP_WITH_EIGEN
#include <Eigen/Core>
#endif
#if NDT_HIP_WITH_PCL
#include <pcl/point_cloud.h>
#include <pcl/registration/registration.h>
#endif
#if NDT_HIP_WITH_GTSAM
#include <gtsam/geometry/Pose3.h>
#endif

namespace ndt_hip {

// same order as pclomp::NeighborSearchMethod (ref: run/pipeline.cpp:471-480)
enum NeighborSearchMethod { KDTREE = NDT_KDTREE, DIRECT26 = NDT_DIRECT26, DIRECT7 = NDT_DIRECT7, DIRECT1 = NDT_DIRECT1 };
// svn_ndt::NeighborSearchMethod (ref: extern/svn_ndt/include/svn_ndt.h:30-35)
enum class SvnNeighborSearchMethod { KDTREE, DIRECT7, DIRECT1 };

// ---- value types ----------------------------------------------------------------------------
#if NDT_HIP_WITH_EIGEN
using Matrix4f = Eigen::Matrix<float, 4, 4>;
using Matrix4d = Eigen::Matrix<double, 4, 4>;
using Matrix6d = Eigen::Matrix<double, 6, 6>;
using Matrix3d = Eigen::Matrix<double, 3, 3>;
using Vector3d = Eigen::Matrix<double, 3, 1>;
#else
// column-major like Eigen's default, same accessors: data(), (r, c), [i]
template <typename T, int R, int C>
struct Mat {
  T m[R * C];
  T* data() { return m; }
  const T* data() const { return m; }
  T& operator()(int r, int c) { return m[c * R + r]; }
  const T& operator()(int r, int c) const { return m[c * R + r]; }
  T& operator[](int i) { return m[i]; }
  const T& operator[](int i) const { return m[i]; }
  bool operator==(const Mat& o) const { return std::equal(m, m + R * C, o.m); }
  bool operator!=(const Mat& o) const { return !(*this == o); }
};
using Matrix4f = Mat<float, 4, 4>;
using Matrix4d = Mat<double, 4, 4>;
using Matrix6d = Mat<double, 6, 6>;
using Matrix3d = Mat<double, 3, 3>;
using Vector3d = Mat<double, 3, 1>;
#endif

namespace detail {
template <class M>
inline M from_rowmajor(const double* a, int rows, int cols) {
  M out;
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) out(r, c) = a[cols * r + c];
  return out;
}
template <class M>
inline void to_rowmajor(const M& in, int rows, int cols, double* a) {
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) a[cols * r + c] = in(r, c);
}
template <class M, class S>
inline M from_colmajor(const S* a, int rows, int cols) {
  M out;
  for (int c = 0; c < cols; ++c)
    for (int r = 0; r < rows; ++r) out(r, c) = a[rows * c + r];
  return out;
}
template <class M, class S>
inline void to_colmajor(const M& in, int rows, int cols, S* a) {
  for (int c = 0; c < cols; ++c)
    for (int r = 0; r < rows; ++r) a[rows * c + r] = (S)in(r, c);
}
// n 4 x 4 matrices of any indexable container -> n x 16 column-major doubles
template <class Poses>
inline std::vector<double> pack_poses(const Poses& poses) {
  std::vector<double> p(16 * poses.size() + 16);
  for (size_t k = 0; k < poses.size(); ++k) to_colmajor(poses[k], 4, 4, &p[16 * k]);
  return p;
}
// anything with matrix() (gtsam::Pose3) as 16 column-major doubles
template <class Pose>
inline auto pose_colmajor(const Pose& p, double a[16]) -> decltype((void)p.matrix()) {
  to_colmajor(p.matrix(), 4, 4, a);
}
}  // namespace detail

inline Matrix4f identity4f() {
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  return detail::from_colmajor<Matrix4f>(I, 4, 4);
}

// pclomp::NdtResult (fields the drivers read: iteration_num, hessian -- run/pipeline.cpp:567-568,
// 594; run/pipeline_ligo_tc.cpp:536-538)
struct NdtResult {
  Matrix4f pose = identity4f();
  float transform_probability = 0.0f;
  float nearest_voxel_transformation_likelihood = 0.0f;
  int iteration_num = 0;
  // [RECALLED: tier4 ndt_omp] entry 0 = the initial guess, then one entry per iteration (no driver reads them)
  std::vector<Matrix4f> transformation_array;
  std::vector<float> transform_probability_array;
  std::vector<float> nearest_voxel_transformation_likelihood_array;
  Matrix6d hessian{};  // of the maximised score: the drivers form cov = -(hessian + 1e-6 I)^-1
  // that covariance, optionally in the block order the drivers hand to GTSAM
  // (ref: run/pipeline.cpp:594-603, src/registercallback.cpp:170-186); false if singular
  bool covarianceForGtsam(Matrix6d& cov, double eps = 1e-6, bool gtsam_order = true) const {
    double h[36], c[36];
    detail::to_rowmajor(hessian, 6, 6, h);
    if (ndt_result_covariance(h, eps, gtsam_order ? 1 : 0, c) != NDT_OK) return false;
    cov = detail::from_rowmajor<Matrix6d>(c, 6, 6);
    return true;
  }
};

// getTargetCells(): what extractNdtData() uses (ref: include/pipeline.hpp:175-206), i.e.
// pclomp::VoxelGridCovariance<PointT>: getLeaves() iterable as {index, leaf} in ascending index
// order, getMinPointPerVoxel(), getLeafCenter(index); Leaf accessors returning Eigen values.
class TargetGrid {
 public:
  struct Leaf {
    ndt_leaf d;
    int getPointCount() const { return d.point_count; }
    Vector3d getMean() const { return detail::from_colmajor<Vector3d>(d.mean, 3, 1); }
    Matrix3d getCov() const { return detail::from_rowmajor<Matrix3d>(d.cov, 3, 3); }
    Matrix3d getInverseCov() const { return detail::from_rowmajor<Matrix3d>(d.icov, 3, 3); }
    Matrix3d getEvecs() const { return detail::from_rowmajor<Matrix3d>(d.evecs, 3, 3); }  // columns = eigenvectors
    Vector3d getEvals() const { return detail::from_colmajor<Vector3d>(d.evals, 3, 1); }
  };
  using Entry = std::pair<size_t, Leaf>;  // {voxel index, leaf}
  const std::vector<Entry>& getLeaves() const { return leaves_; }
  int getMinPointPerVoxel() const { return min_points_; }
  // O(log V): the leaves are kept in ascending index order.  Like the reference's getLeaf(index), only a VALID leaf is
  // handed out -- at least getMinPointPerVoxel() points (a leaf whose covariance could not be inverted carries -1; ref:
  // voxel_grid_covariance.h:262-278).  (The engine exports the valid leaves only, so getLeaves() iterates over those; the
  // reference's map also holds the voxels with too few points, which its users filter out: include/pipeline.hpp:186.)
  const Leaf* getLeaf(size_t index) const {
    auto it = std::lower_bound(leaves_.begin(), leaves_.end(), index,
                               [](const Entry& e, size_t i) { return e.first < i; });
    return (it != leaves_.end() && it->first == index && it->second.d.point_count >= min_points_) ? &it->second : nullptr;
  }
  Vector3d getLeafCenter(size_t index) const {
    double c[3] = {0.0, 0.0, 0.0};
    if (const Leaf* l = getLeaf(index))
      for (int a = 0; a < 3; ++a) c[a] = (double)l->d.center[a];
    return detail::from_colmajor<Vector3d>(c, 3, 1);
  }

  // ---- the reference grid's query surface (round 5; ref: extern/svn_ndt/include/voxel_grid_covariance.h:194-200,280-381,
  // voxel_grid_covariance_impl.hpp:46-71,455-615), answered on the host from the exported leaves and the grid geometry --
  // the same f32 bounds test and index arithmetic, so a query lands in the voxel the engine's kernels put it in.  Points
  // are anything with x / y / z members (pcl::PointXYZ, PointXYZI, the PCL-free point types of this header) or
  // operator[] (Eigen::Vector3f).  No driver calls these; they exist so that code written against the reference's grid
  // class keeps compiling.
  using LeafConstPtr = const Leaf*;
  double getCovEigValueInflationRatio() const { return eig_ratio_; }
  bool isPointWithinBounds(float px, float py, float pz) const {   // ref: voxel_grid_covariance_impl.hpp:46-71
    if (gi_.inverse_leaf_size == 0.0f) return false;
    const float w = gi_.leaf_size;
    return px >= (float)gi_.min_b[0] * w && px < (float)(gi_.max_b[0] + 1) * w && py >= (float)gi_.min_b[1] * w &&
           py < (float)(gi_.max_b[1] + 1) * w && pz >= (float)gi_.min_b[2] * w && pz < (float)(gi_.max_b[2] + 1) * w;
  }
  LeafConstPtr getLeafAt(float px, float py, float pz) const {    // ref: voxel_grid_covariance.h:280-303
    if (!isPointWithinBounds(px, py, pz)) return nullptr;
    const float il = gi_.inverse_leaf_size;
    const int i0 = static_cast<int>(std::floor(px * il) - (float)gi_.min_b[0]);
    const int i1 = static_cast<int>(std::floor(py * il) - (float)gi_.min_b[1]);
    const int i2 = static_cast<int>(std::floor(pz * il) - (float)gi_.min_b[2]);
    return getLeaf(static_cast<size_t>(i0 + i1 * gi_.div_b[0] + i2 * gi_.div_b[0] * gi_.div_b[1]));
  }
  template <class P>
  auto getLeaf(const P& p) const -> decltype((void)p.x, LeafConstPtr()) { return getLeafAt(p.x, p.y, p.z); }
  template <class V>
  auto getLeaf(const V& v) const -> decltype((void)v[0], (void)v.data(), LeafConstPtr()) { return getLeafAt((float)v[0], (float)v[1], (float)v[2]); }
  // DIRECT7 / DIRECT1 (ref: voxel_grid_covariance_impl.hpp:560-615): the point offset by +-leaf in f32 and re-classified
  template <class P>
  int getNeighborhoodAtPoint7(const P& ref, std::vector<LeafConstPtr>& neighbors) const {
    neighbors.clear();
    neighbors.reserve(7);
    const float w = gi_.leaf_size, x = ref.x, y = ref.y, z = ref.z;
    if (LeafConstPtr c = getLeafAt(x, y, z)) neighbors.push_back(c);
    if (!(w > 0.0f)) return (int)neighbors.size();
    const float probe[6][3] = {{x + w, y, z}, {x - w, y, z}, {x, y + w, z}, {x, y - w, z}, {x, y, z + w}, {x, y, z - w}};
    for (const auto& q : probe)
      if (LeafConstPtr l = getLeafAt(q[0], q[1], q[2])) neighbors.push_back(l);
    return (int)neighbors.size();
  }
  template <class P>
  int getNeighborhoodAtPoint1(const P& ref, std::vector<LeafConstPtr>& neighbors) const {
    neighbors.clear();
    if (LeafConstPtr l = getLeafAt(ref.x, ref.y, ref.z)) neighbors.push_back(l);
    return (int)neighbors.size();
  }
  // the centroid cloud the reference's kd-tree is built on: the f32-rounded means of the valid leaves, ascending voxel
  // index (ref: voxel_grid_covariance_impl.hpp:400-440)
  struct Centroid { float x, y, z; };
  const std::vector<Centroid>& getCentroids() const {
    if (!centroids_built_) {
      centroids_.clear();
      centroid_leaf_.clear();
      for (size_t i = 0; i < leaves_.size(); ++i) {
        const ndt_leaf& d = leaves_[i].second.d;
        if (d.point_count < min_points_) continue;
        centroids_.push_back(Centroid{(float)d.mean[0], (float)d.mean[1], (float)d.mean[2]});
        centroid_leaf_.push_back(i);
      }
      centroids_built_ = true;
    }
    return centroids_;
  }
  // FLANN's L2_Simple in f32 (accumulated x, y, z), strict `<` on the squared radius, results by ascending distance -- what
  // pcl::KdTreeFLANN::radiusSearch returns (ref: voxel_grid_covariance_impl.hpp:505-554).  A linear scan of the centroids: a
  // host-side convenience, not the engine's KDTREE path (that one is the 27-cell scan inside k_derivatives).
  template <class P>
  int radiusSearch(const P& point, double radius, std::vector<LeafConstPtr>& k_leaves, std::vector<float>& k_sqr_distances,
                   unsigned int max_nn = 0) const {
    k_leaves.clear();
    k_sqr_distances.clear();
    if (radius <= 0.0) return 0;
    const float r2 = (float)(radius * radius);
    std::vector<std::pair<float, size_t>> hits;
    const std::vector<Centroid>& c = getCentroids();
    for (size_t i = 0; i < c.size(); ++i) {
      const float d = sqr_distance(c[i], point.x, point.y, point.z);
      if (d < r2) hits.emplace_back(d, i);
    }
    std::sort(hits.begin(), hits.end());
    if (max_nn > 0 && hits.size() > max_nn) hits.resize(max_nn);
    for (const auto& h : hits) { k_leaves.push_back(&leaves_[centroid_leaf_[h.second]].second); k_sqr_distances.push_back(h.first); }
    return (int)k_leaves.size();
  }
  template <class P>
  int nearestKSearch(const P& point, int k, std::vector<LeafConstPtr>& k_leaves, std::vector<float>& k_sqr_distances) const {
    k_leaves.clear();
    k_sqr_distances.clear();
    if (k <= 0) return 0;
    std::vector<std::pair<float, size_t>> all;
    const std::vector<Centroid>& c = getCentroids();
    all.reserve(c.size());
    for (size_t i = 0; i < c.size(); ++i) all.emplace_back(sqr_distance(c[i], point.x, point.y, point.z), i);
    const size_t n = std::min(all.size(), (size_t)k);
    std::partial_sort(all.begin(), all.begin() + n, all.end());
    for (size_t i = 0; i < n; ++i) { k_leaves.push_back(&leaves_[centroid_leaf_[all[i].second]].second); k_sqr_distances.push_back(all[i].first); }
    return (int)n;
  }

  std::vector<Entry> leaves_;
  int min_points_ = 6;
  ndt_grid_info gi_{};          // geometry of the grid the leaves were exported from
  double eig_ratio_ = 0.01;

 private:
  static float sqr_distance(const Centroid& c, float px, float py, float pz) {
    const float ex = px - c.x, ey = py - c.y, ez = pz - c.z;
    float d = ex * ex;
    d = d + ey * ey;
    d = d + ez * ez;
    return d;
  }
  mutable std::vector<Centroid> centroids_;
  mutable std::vector<size_t> centroid_leaf_;   // centroid -> position in leaves_
  mutable bool centroids_built_ = false;
};

#if NDT_HIP_WITH_PCL
template <typename PointT>
using PointCloud = pcl::PointCloud<PointT>;
#else
template <typename PointT>
struct PointCloud {
  using Ptr = std::shared_ptr<PointCloud<PointT>>;
  using ConstPtr = std::shared_ptr<const PointCloud<PointT>>;
  std::vector<PointT> points;
  size_t size() const { return points.size(); }
  bool empty() const { return points.empty(); }
};
struct PointXYZ { float x, y, z, pad; };                        // 16 bytes like pcl::PointXYZ
struct PointXYZI { float x, y, z, pad; float intensity, p1, p2, p3; };  // 32 bytes like pcl::PointXYZI
#endif

// The complete state of a map's occupied voxels, ascending (k, j, i): what a caller saves at shutdown, loads at the
// next start (mapReset with the same leaf, mapEnableMoments if `moments` is filled, mapImportState) or merges into
// another map.  The sums are the map's own, not divided by the count.  File formats are the caller's business.
struct MapState {
  float leaf = 0.0f;
  bool with_intensity = false;
  std::vector<int32_t> ijk;      // 3 per voxel
  std::vector<int32_t> counts;   // 1 per voxel
  std::vector<float> sums;       // 4 per voxel: sum x, y, z, intensity
  std::vector<double> moments;   // 9 per voxel (x y z xx xy xz yy yz zz); empty for a map without moments
  size_t size() const { return counts.size(); }
};

template <typename PointSource, typename PointTarget>
class NormalDistributionsTransform
#if NDT_HIP_WITH_PCL
    : public pcl::Registration<PointSource, PointTarget>
#endif
{
 public:
  using PointCloudSource = PointCloud<PointSource>;
  using PointCloudTarget = PointCloud<PointTarget>;
#if NDT_HIP_WITH_PCL
  // whatever smart pointer this PCL uses (std:: since 1.11, boost:: before), so that
  // `registerCallback.registration = ndt_omp;` (ref: run/pipeline.cpp:481) converts
  using Base = pcl::Registration<PointSource, PointTarget>;
  using Ptr = typename std::pointer_traits<typename Base::Ptr>::template rebind<NormalDistributionsTransform<PointSource, PointTarget>>;
  using ConstPtr = typename std::pointer_traits<typename Base::Ptr>::template rebind<const NormalDistributionsTransform<PointSource, PointTarget>>;
#else
  using Ptr = std::shared_ptr<NormalDistributionsTransform<PointSource, PointTarget>>;
  using ConstPtr = std::shared_ptr<const NormalDistributionsTransform<PointSource, PointTarget>>;
#endif

  NormalDistributionsTransform() {
    ndt_default_params(&prm_);
    status_ = ndt_create(&prm_, &h_);
#if NDT_HIP_WITH_PCL
    this->reg_name_ = "ndt_hip::NormalDistributionsTransform";
    this->max_iterations_ = prm_.max_iterations;
    this->transformation_epsilon_ = prm_.trans_epsilon;
#endif
  }
  ~NormalDistributionsTransform() { ndt_destroy(h_); }
  NormalDistributionsTransform(const NormalDistributionsTransform&) = delete;
  NormalDistributionsTransform& operator=(const NormalDistributionsTransform&) = delete;

  // ---- pclomp setters (ref: run/pipeline.cpp:467-480, run/pipeline_ligo_tc.cpp:293) ----
  void setNumThreads(int n) { prm_.num_threads = n; push(); }
  int getNumThreads() const { return prm_.num_threads; }
  void setResolution(float r) { prm_.resolution = r; push(); }
  float getResolution() const { return prm_.resolution; }
  void setStepSize(double s) { prm_.step_size = s; push(); }
  double getStepSize() const { return prm_.step_size; }
  void setOutlierRatio(double o) { prm_.outlier_ratio = o; push(); }
  double getOulierRatio() const { return prm_.outlier_ratio; }  // sic, the PCL spelling
  void setNeighborhoodSearchMethod(NeighborSearchMethod m) { prm_.search_method = (int)m; push(); }
  NeighborSearchMethod getNeighborhoodSearchMethod() const { return (NeighborSearchMethod)prm_.search_method; }
  void setRegularizationScaleFactor(float k) { prm_.regularization_scale_factor = k; push(); }
  void setMinPointPerVoxel(int n) { prm_.min_points_per_voxel = n; push(); }
  void setTransformationEpsilon(double e) {
#if NDT_HIP_WITH_PCL
    this->transformation_epsilon_ = e;
#endif
    prm_.trans_epsilon = e;
    push();
  }
  void setMaximumIterations(int n) {
#if NDT_HIP_WITH_PCL
    this->max_iterations_ = n;
#endif
    prm_.max_iterations = n;
    push();
  }
  void setRegularizationPose(const Matrix4f& T) {  // ref: run/pipeline_ligo_tc.cpp:531
    float a[16];
    detail::to_colmajor(T, 4, 4, a);
    status_ = h_ ? ndt_set_regularization_pose(h_, a) : NDT_ERR_NO_DEVICE;
  }
  void unsetRegularizationPose() { status_ = h_ ? ndt_clear_regularization_pose(h_) : NDT_ERR_NO_DEVICE; }
  // every engine parameter at once (hessian_mode, cov_mode, add_ridge, use_line_search, ...)
  const ndt_params& params() const { return prm_; }
  void setParams(const ndt_params& p) { const int dev = prm_.device_id; prm_ = p; prm_.device_id = dev; push(); }

  // ---- clouds ----
#if NDT_HIP_WITH_PCL
  void setInputTarget(const typename Base::PointCloudTargetConstPtr& cloud) override {
    Base::setInputTarget(cloud);
    // pcl::Registration::initCompute() would build a FLANN kd-tree over the whole target on the
    // next align() (hundreds of ms for a 1M-point map); NDT never queries it
    this->target_cloud_updated_ = false;
    uploadTarget(cloud.get());
  }
  void setInputSource(const typename Base::PointCloudSourceConstPtr& cloud) override {
    Base::setInputSource(cloud);
    this->source_cloud_updated_ = false;
    uploadSource(cloud.get());
  }
#else
  void setInputTarget(const typename PointCloudTarget::ConstPtr& cloud) { uploadTarget(cloud.get()); }
  void setInputSource(const typename PointCloudSource::ConstPtr& cloud) { uploadSource(cloud.get()); }
#endif

  // ---- registration ----
  // public in pclomp too (ref: extern/svn_ndt/test/test_svn_ndt.cpp:171); called by
  // pcl::Registration::align(output, guess) in the PCL face
  void computeTransformation(PointCloudSource& output, const Matrix4f& guess)
#if NDT_HIP_WITH_PCL
      override
#endif
  {
    float g[16];
    detail::to_colmajor(guess, 4, 4, g);
    run(g);
#if NDT_HIP_WITH_PCL
    this->final_transformation_ = detail::from_colmajor<Matrix4f>(res_.final_transformation, 4, 4);
    this->transformation_ = this->final_transformation_;
    this->converged_ = res_.converged != 0;
    this->nr_iterations_ = res_.iterations;
#endif
    fillOutput(output);
  }
#if !NDT_HIP_WITH_PCL
  void align(PointCloudSource& output, const Matrix4f& guess = identity4f()) { computeTransformation(output, guess); }
  Matrix4f getFinalTransformation() const { return detail::from_colmajor<Matrix4f>(res_.final_transformation, 4, 4); }
  bool hasConverged() const { return res_.converged != 0; }
#endif
  int getFinalNumIteration() const { return res_.iterations; }
  double getTransformationProbability() const { return res_.transform_probability; }
  double getNearestVoxelTransformationLikelihood() const { return res_.nearest_voxel_transformation_likelihood; }
  // pcl::Registration::getFitnessScore(max_range) [RECALLED]: mean squared distance from the source, moved by the last
  // align's final transformation (identity before any align), to the nearest raw target point, over the points with
  // d^2 <= max_range (a squared distance) -- on the device (ndt_fitness_score).  PCL's own method is not virtual: it
  // searches the kd-tree this adapter never lets PCL build, so call this one on the adapter type, not through a
  // pcl::Registration pointer.  On error: DBL_MAX, and lastStatus() says why.
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return std::numeric_limits<double>::max(); }
    float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (aligned_) std::memcpy(T, res_.final_transformation, sizeof(T));
    ndt_fitness f;
    status_ = ndt_fitness_score(h_, T, max_range, &f, nullptr, 0);
    return status_ == NDT_OK ? f.fitness_score : std::numeric_limits<double>::max();
  }

  // scoring-only calls of pclomp: score of `cloud` under transform T against the
  // current target, no gradient, nothing about the engine's source / result changes except the
  // source cloud (replaced by `cloud`, as pclomp's versions take the cloud to score)
  template <class Cloud>
  double calculateTransformationProbability(const Cloud& cloud, const Matrix4f& T = identity4f()) {
    ndt_score s;
    return scoreCloud(cloud, T, &s) ? s.transform_probability : 0.0;
  }
  template <class Cloud>
  double calculateNearestVoxelTransformationLikelihood(const Cloud& cloud, const Matrix4f& T = identity4f()) {
    ndt_score s;
    return scoreCloud(cloud, T, &s) ? s.nearest_voxel_transformation_likelihood : 0.0;
  }

  // ---- per-point scores (ndt_score_points) and the score-based source filter (ndt_filter_source) ----
  // what a scoring-only evaluation of the CURRENT source under T adds up, per point in the order the source was handed
  // over; best_voxel is a TargetGrid leaf index (-1: no voxel contributed).  On error: empty arrays, lastStatus() says why.
  struct PointScores {
    std::vector<double> score, nearest_voxel_score;
    std::vector<int32_t> n_neighbors;
    std::vector<int64_t> best_voxel;
    size_t size() const { return score.size(); }
  };
  PointScores scorePoints(const Matrix4f& T = identity4f()) {
    PointScores ps;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return ps; }
    const int64_t n = ndt_source_size(h_);
    if (n < 0) { status_ = (int)n; return ps; }
    float a[16];
    detail::to_colmajor(T, 4, 4, a);
    ps.score.resize((size_t)n); ps.nearest_voxel_score.resize((size_t)n); ps.n_neighbors.resize((size_t)n); ps.best_voxel.resize((size_t)n);
    status_ = ndt_score_points(h_, a, ps.score.data(), ps.nearest_voxel_score.data(), ps.n_neighbors.data(), ps.best_voxel.data(), (size_t)n);
    if (status_ != NDT_OK) ps = PointScores();
    return ps;
  }
  // the current source moved by T (ndt_transform_source) with intensity = the point's nearest_voxel_score: the shape of
  // tier4 ndt_omp's calculateNearestVoxelScoreEachPoint [RECALLED], which colours a scan by how well the map explains it
  template <class PointOut = PointSource>
  PointCloud<PointOut> nearestVoxelScoreEachPoint(const Matrix4f& T = identity4f()) {
    PointCloud<PointOut> out;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return out; }
    const int64_t n = ndt_source_size(h_);
    if (n < 0) { status_ = (int)n; return out; }
    float a[16];
    detail::to_colmajor(T, 4, 4, a);
    std::vector<double> nvs((size_t)n);
    std::vector<float> xyz(3 * (size_t)n);
    status_ = ndt_score_points(h_, a, nullptr, nvs.data(), nullptr, nullptr, (size_t)n);
    if (status_ == NDT_OK && n > 0) status_ = ndt_transform_source(h_, a, xyz.data(), (size_t)n);
    if (status_ != NDT_OK) return out;
    out.points.resize((size_t)n);
    for (size_t i = 0; i < (size_t)n; ++i) {
      out.points[i].x = xyz[3 * i];
      out.points[i].y = xyz[3 * i + 1];
      out.points[i].z = xyz[3 * i + 2];
      out.points[i].intensity = (float)nvs[i];
    }
    return out;
  }
  // tier4's own signature [RECALLED]: `cloud` is already in the map frame; it becomes the engine's source, as with the
  // other scoring-only calls above
  template <class Cloud>
  PointCloud<PointSource> calculateNearestVoxelScoreEachPoint(const Cloud& cloud) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return PointCloud<PointSource>(); }
    uploadSource(&cloud);
    if (status_ != NDT_OK) return PointCloud<PointSource>();
    return nearestVoxelScoreEachPoint<PointSource>(identity4f());
  }
  // the source points (as handed over, not transformed) whose nearest_voxel_score under T is >= min_score (keep_below:
  // those below it, points without a neighbour included), in input order; `index` (nullable) receives their positions
  PointCloud<PointSource> filterSource(const Matrix4f& T, double min_score, bool keep_below = false,
                                       std::vector<int32_t>* index = nullptr) {
    PointCloud<PointSource> out;
    if (index) index->clear();
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return out; }
    const int64_t n = ndt_source_size(h_);
    if (n < 0) { status_ = (int)n; return out; }
    float a[16];
    detail::to_colmajor(T, 4, 4, a);
    std::vector<float> xyz(3 * (size_t)n + 3);
    std::vector<int32_t> idx((size_t)n + 1);
    size_t m = 0;
    status_ = ndt_filter_source(h_, a, min_score, keep_below ? 1 : 0, xyz.data(), idx.data(), (size_t)n, &m);
    if (status_ != NDT_OK) return out;
    out.points.resize(m);   // value-initialised points: the fields the engine does not write keep their defaults
    for (size_t i = 0; i < m; ++i) {
      out.points[i].x = xyz[3 * i];
      out.points[i].y = xyz[3 * i + 1];
      out.points[i].z = xyz[3 * i + 2];
    }
    if (index) index->assign(idx.begin(), idx.begin() + (std::ptrdiff_t)m);
    return out;
  }

  NdtResult getResult() const {
    NdtResult r;
    r.pose = detail::from_colmajor<Matrix4f>(res_.final_transformation, 4, 4);
    r.transform_probability = (float)res_.transform_probability;
    r.nearest_voxel_transformation_likelihood = (float)res_.nearest_voxel_transformation_likelihood;
    r.iteration_num = res_.iterations;
    r.hessian = detail::from_rowmajor<Matrix6d>(res_.hessian, 6, 6);
    const int n = h_ ? ndt_get_iteration_history(h_, nullptr, nullptr, nullptr, 0) : 0;
    if (n > 0) {
      std::vector<float> T((size_t)n * 16);
      std::vector<double> tp((size_t)n), nv((size_t)n);
      ndt_get_iteration_history(h_, T.data(), tp.data(), nv.data(), n);
      for (int i = 0; i < n; ++i) {
        r.transformation_array.push_back(detail::from_colmajor<Matrix4f>(T.data() + 16 * (size_t)i, 4, 4));
        r.transform_probability_array.push_back((float)tp[(size_t)i]);
        r.nearest_voxel_transformation_likelihood_array.push_back((float)nv[(size_t)i]);
      }
    }
    return r;
  }

  // align() from each of K guesses (1 <= K <= 256) in shared launches (ndt_align_batch): one result per guess, its final
  // transformation in `pose` as getResult().pose holds it after align().  The adapter's own result -- getFinalTransformation,
  // hasConverged, getResult and its iteration arrays -- stays that of the last align(); the results here carry no iteration
  // arrays.  lastStatus() reports this call; on an error every result holds its guess.
  std::vector<NdtResult> alignMany(const std::vector<Matrix4f>& guesses) {
    const size_t K = guesses.size();
    std::vector<float> g(16 * (K ? K : 1));
    for (size_t k = 0; k < K; ++k) detail::to_colmajor(guesses[k], 4, 4, &g[16 * k]);
    std::vector<ndt_result> raw(K ? K : 1);
    status_ = h_ ? ndt_align_batch(h_, g.data(), (int)K, raw.data()) : NDT_ERR_NO_DEVICE;
    std::vector<NdtResult> out(K);
    for (size_t k = 0; k < K; ++k) {
      if (status_ != NDT_OK) {  // the reference returns the prior, not converged
        std::memset(&raw[k], 0, sizeof(raw[k]));
        std::memcpy(raw[k].final_transformation, &g[16 * k], sizeof(float) * 16);
      }
      out[k].pose = detail::from_colmajor<Matrix4f>(raw[k].final_transformation, 4, 4);
      out[k].transform_probability = (float)raw[k].transform_probability;
      out[k].nearest_voxel_transformation_likelihood = (float)raw[k].nearest_voxel_transformation_likelihood;
      out[k].iteration_num = raw[k].iterations;
      out[k].hessian = detail::from_rowmajor<Matrix6d>(raw[k].hessian, 6, 6);
    }
    return out;
  }

  // ---- voxel grid (ref: include/pipeline.hpp:178-206) ----
  const TargetGrid& getTargetCells() {
    ndt_grid_info gi;
    grid_ = TargetGrid();
    grid_.min_points_ = prm_.min_points_per_voxel < 3 ? 3 : prm_.min_points_per_voxel;
    grid_.eig_ratio_ = prm_.eig_inflation_ratio;
    if (h_ && ndt_get_grid_info(h_, &gi) == NDT_OK && gi.n_leaves > 0) {
      grid_.gi_ = gi;
      std::vector<ndt_leaf> buf((size_t)gi.n_leaves);
      const int64_t n = ndt_export_leaves(h_, buf.data(), buf.size());  // ascending index
      grid_.leaves_.reserve(n > 0 ? (size_t)n : 0);
      for (int64_t i = 0; i < n; ++i) grid_.leaves_.emplace_back((size_t)buf[i].index, TargetGrid::Leaf{buf[i]});
    }
    return grid_;
  }

  // ---- pcl::VoxelGrid on the device (ref: run/pipeline_ins_map_distribution.cpp:324-340: vg.setLeafSize(vs, vs, vs);
  // vg.setInputCloud(map); vg.filter(*ds_map)) ----
  // `out` receives the centroid (x, y, z and, for point types with an `intensity` member at byte 16, the intensity) of
  // every occupied voxel in ascending voxel index; the engine's target and source are left as they are
  template <class P>
  static auto intensity_offset_of(int) -> decltype((void)static_cast<const float*>(&std::declval<const P&>().intensity), int()) {
    static const P probe{};
    return (int)(reinterpret_cast<const char*>(&probe.intensity) - reinterpret_cast<const char*>(&probe.x));
  }
  template <class P>
  static int intensity_offset_of(long) { return -1; }

  template <class Cloud>
  void voxelDownsample(const Cloud& in, float leaf, Cloud& out) {
    out.points.clear();
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    if (in.points.empty()) { status_ = NDT_OK; return; }
    using P = typename std::decay<decltype(in.points[0])>::type;
    out.points.resize(in.points.size());   // value-initialised points: the fields the engine does not write keep their defaults
    size_t m = 0;
    // the intensity is averaged only for point types that HAVE a float member of that name, at ITS offset (pcl::PointXYZRGB
    // and PointNormal are 32 bytes too and carry packed colour / a normal at byte 16: never averaged as a float)
    status_ = ndt_voxel_downsample(h_, &in.points[0].x, in.points.size(), sizeof(P), intensity_offset_of<P>(0), leaf,
                                   &out.points[0].x, out.points.size(), &m);
    out.points.resize(status_ == NDT_OK ? m : 0);
  }

  // ---- sparse voxel map accumulated scan by scan (ref: run/pipeline_ins_map_distribution.cpp:281-377: cumm_thread
  // transforms every keyframe scan into the map frame and keeps it; the shutdown path filters the concatenation) ----
  // not part of pclomp: the map keeps per-voxel sums in HBM instead of the points, mapExport returns what
  // voxelDownsample returns for the concatenation of everything added (pose: 16 column-major doubles, or null)
  void mapReset(float leaf, bool with_intensity = false, int64_t initial_capacity = 0) {
    status_ = h_ ? ndt_map_reset(h_, leaf, with_intensity ? 1 : 0, initial_capacity) : NDT_ERR_NO_DEVICE;
  }
  void mapClear() { status_ = h_ ? ndt_map_clear(h_) : NDT_ERR_NO_DEVICE; }
  template <class Cloud>
  void mapAdd(const Cloud& cloud, const double* pose_colmajor = nullptr) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    if (cloud.points.empty()) { status_ = ndt_map_add(h_, nullptr, 0, 12, -1, pose_colmajor); return; }
    using P = typename std::decay<decltype(cloud.points[0])>::type;
    status_ = ndt_map_add(h_, &cloud.points[0].x, cloud.points.size(), sizeof(P), intensity_offset_of<P>(0), pose_colmajor);
  }
  void mapAddDevice(const float* dx, const float* dy, const float* dz, const float* d_intensity, size_t n,
                    const double* pose_colmajor = nullptr) {
    status_ = h_ ? ndt_map_add_device(h_, dx, dy, dz, d_intensity, n, pose_colmajor) : NDT_ERR_NO_DEVICE;
  }
  void mapAddKeyframe(int64_t id, const double* pose_colmajor) {
    status_ = h_ ? ndt_map_add_keyframe(h_, id, pose_colmajor) : NDT_ERR_NO_DEVICE;
  }
  ndt_map_info mapInfo() {
    ndt_map_info mi{};
    status_ = h_ ? ndt_map_get_info(h_, &mi) : NDT_ERR_NO_DEVICE;
    return mi;
  }
  // one point per voxel with >= min_points points, ascending (k, j, i); counts: the voxels' point counts, if asked for
  template <class Cloud>
  void mapExport(Cloud& out, int min_points = 1, std::vector<int32_t>* counts = nullptr) {
    out.points.clear();
    if (counts) counts->clear();
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    ndt_map_info mi{};
    status_ = ndt_map_get_info(h_, &mi);
    if (status_ != NDT_OK || mi.n_voxels == 0) return;
    using P = typename std::decay<decltype(out.points[0])>::type;
    out.points.resize((size_t)mi.n_voxels);
    std::vector<int32_t> cnt((size_t)mi.n_voxels);
    size_t m = 0;
    status_ = ndt_map_export(h_, min_points, &out.points[0].x, sizeof(P), intensity_offset_of<P>(0), cnt.data(),
                             out.points.size(), &m);
    out.points.resize(status_ == NDT_OK ? m : 0);
    if (counts && status_ == NDT_OK) counts->assign(cnt.begin(), cnt.begin() + (long)m);
  }
  size_t mapExportDevice(float* ox, float* oy, float* oz, float* o_intensity, int32_t* o_count, size_t cap, int min_points = 1) {
    size_t m = 0;
    status_ = h_ ? ndt_map_export_device(h_, min_points, ox, oy, oz, o_intensity, o_count, cap, &m) : NDT_ERR_NO_DEVICE;
    return m;
  }
  void setInputTargetFromMap(int min_points = 1) {
    status_ = h_ ? ndt_set_target_from_map(h_, min_points) : NDT_ERR_NO_DEVICE;
  }
  // per-voxel moments (the nine f64 sums of the target build) and the target made directly from them: right after
  // mapReset; mapExportMoments fills ijk (3 per voxel), counts and sums (9 per voxel: x y z xx xy xz yy yz zz)
  void mapEnableMoments() { status_ = h_ ? ndt_map_enable_moments(h_) : NDT_ERR_NO_DEVICE; }
  bool mapHasMoments() const { return h_ && ndt_map_has_moments(h_) == 1; }
  void mapExportMoments(std::vector<int32_t>& ijk, std::vector<int32_t>& counts, std::vector<double>& sums, int min_points = 1) {
    ijk.clear(); counts.clear(); sums.clear();
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    ndt_map_info mi{};
    status_ = ndt_map_get_info(h_, &mi);
    if (status_ != NDT_OK) return;
    const size_t cap = (size_t)mi.n_voxels;
    ijk.resize(3 * cap); counts.resize(cap); sums.resize(9 * cap);
    size_t m = 0;
    status_ = ndt_map_export_moments(h_, min_points, ijk.data(), counts.data(), sums.data(), cap, &m);
    if (status_ != NDT_OK) m = 0;
    ijk.resize(3 * m); counts.resize(m); sums.resize(9 * m);
  }
  // box_min / box_max: three floats each, or both null for the whole map
  void setInputTargetFromMapMoments(const float* box_min = nullptr, const float* box_max = nullptr) {
    status_ = h_ ? ndt_set_target_from_map_moments(h_, box_min, box_max) : NDT_ERR_NO_DEVICE;
  }

  // ---- the map bounded, kept and combined (ndt_map_crop, ndt_map_export_state, ndt_map_import_state) ----
  // keeps the voxels inside the box (remove_inside: drops them and keeps the rest); returns the number of voxels dropped
  int64_t mapCrop(const float box_min[3], const float box_max[3], bool remove_inside = false) {
    int64_t removed = 0;
    status_ = h_ ? ndt_map_crop(h_, box_min, box_max, remove_inside ? 1 : 0, &removed) : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? removed : 0;
  }
  // ---- free-space carving (ndt_map_carve*): the voxels that the rays of a scan pass through, and none ends in, go.
  // origin: the sensor position in the cloud's own frame (the pose moves it with the points; null pose: as it is);
  // params null: ndt_map_carve_default_params.  Returns the call's counts (all zero on error, lastStatus() says why). ----
  template <class Cloud>
  ndt_map_carve_result mapCarve(const Cloud& cloud, const float origin[3], const double* pose_colmajor = nullptr,
                                const ndt_map_carve_params* params = nullptr) {
    ndt_map_carve_result r{};
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return r; }
    ndt_map_carve_params def;
    ndt_map_carve_default_params(&def);
    if (cloud.points.empty()) status_ = ndt_map_carve(h_, nullptr, 0, 12, origin, pose_colmajor, params ? params : &def, &r);
    else status_ = ndt_map_carve(h_, &cloud.points[0].x, cloud.points.size(), sizeof(cloud.points[0]), origin, pose_colmajor,
                                 params ? params : &def, &r);
    return status_ == NDT_OK ? r : ndt_map_carve_result{};
  }
  ndt_map_carve_result mapCarveDevice(const float* dx, const float* dy, const float* dz, size_t n, const float origin[3],
                                      const double* pose_colmajor = nullptr, const ndt_map_carve_params* params = nullptr) {
    ndt_map_carve_result r{};
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return r; }
    ndt_map_carve_params def;
    ndt_map_carve_default_params(&def);
    status_ = ndt_map_carve_device(h_, dx, dy, dz, n, origin, pose_colmajor, params ? params : &def, &r);
    return status_ == NDT_OK ? r : ndt_map_carve_result{};
  }
  ndt_map_carve_result mapCarveKeyframe(int64_t id, const float origin[3], const double* pose_colmajor,
                                        const ndt_map_carve_params* params = nullptr) {
    ndt_map_carve_result r{};
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return r; }
    ndt_map_carve_params def;
    ndt_map_carve_default_params(&def);
    status_ = ndt_map_carve_keyframe(h_, id, origin, pose_colmajor, params ? params : &def, &r);
    return status_ == NDT_OK ? r : ndt_map_carve_result{};
  }
  // ---- connected components (ndt_map_components*): which voxels belong together under 6 / 18 / 26 adjacency; voxels with
  // fewer than min_count points take no part.  params null: ndt_map_components_default_params (26, 1).  On error the
  // outputs are empty / zero and lastStatus() says why. ----
  ndt_map_components_info mapComponents(const ndt_map_components_params* params = nullptr) {
    ndt_map_components_info info{};
    info.largest = -1;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return info; }
    ndt_map_components_params def;
    ndt_map_components_default_params(&def);
    status_ = ndt_map_components(h_, params ? params : &def, &info);
    return info;
  }
  // the component table in index order
  void mapExportComponents(std::vector<ndt_map_component>& comps, const ndt_map_components_params* params = nullptr) {
    comps.clear();
    const ndt_map_components_info info = mapComponents(params);
    if (status_ != NDT_OK) return;
    ndt_map_components_params def;
    ndt_map_components_default_params(&def);
    comps.resize((size_t)info.n_components);
    size_t m = 0;
    status_ = ndt_map_export_components(h_, params ? params : &def, comps.data(), comps.size(), &m);
    comps.resize(status_ == NDT_OK ? m : 0);
  }
  // every occupied voxel in mapExportState's order: ijk (3 per voxel) and label (-1: fewer than min_count points)
  void mapExportLabels(std::vector<int32_t>& ijk, std::vector<int32_t>& labels, const ndt_map_components_params* params = nullptr) {
    ijk.clear(); labels.clear();
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    ndt_map_info mi{};
    status_ = ndt_map_get_info(h_, &mi);
    if (status_ != NDT_OK) return;
    ndt_map_components_params def;
    ndt_map_components_default_params(&def);
    const size_t cap = (size_t)mi.n_voxels;
    ijk.resize(3 * cap); labels.resize(cap);
    size_t m = 0;
    status_ = ndt_map_export_labels(h_, params ? params : &def, ijk.data(), labels.data(), cap, &m);
    if (status_ != NDT_OK) m = 0;
    ijk.resize(3 * m); labels.resize(m);
  }
  // into device arrays of cap rows (either may be null); returns the number of voxels
  size_t mapExportLabelsDevice(int32_t* d_ijk, int32_t* d_label, size_t cap, const ndt_map_components_params* params = nullptr) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return 0; }
    ndt_map_components_params def;
    ndt_map_components_default_params(&def);
    size_t m = 0;
    status_ = ndt_map_export_labels_device(h_, params ? params : &def, d_ijk, d_label, cap, &m);
    return m;
  }
  // the label of the map voxel each point falls in once moved by the pose (as mapAdd moves it), -1 where there is none;
  // returns the number of points with a label
  template <class Cloud>
  int64_t mapLabelPoints(const Cloud& cloud, std::vector<int32_t>& labels, const double* pose_colmajor = nullptr,
                         const ndt_map_components_params* params = nullptr) {
    labels.assign(cloud.points.size(), -1);
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return 0; }
    ndt_map_components_params def;
    ndt_map_components_default_params(&def);
    int64_t k = 0;
    if (cloud.points.empty()) status_ = ndt_map_label_points(h_, params ? params : &def, nullptr, 0, 12, pose_colmajor, nullptr, &k);
    else status_ = ndt_map_label_points(h_, params ? params : &def, &cloud.points[0].x, cloud.points.size(), sizeof(cloud.points[0]),
                                        pose_colmajor, labels.data(), &k);
    return status_ == NDT_OK ? k : 0;
  }
  int64_t mapLabelPointsDevice(const float* dx, const float* dy, const float* dz, size_t n, int32_t* d_label,
                               const double* pose_colmajor = nullptr, const ndt_map_components_params* params = nullptr) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return 0; }
    ndt_map_components_params def;
    ndt_map_components_default_params(&def);
    int64_t k = 0;
    status_ = ndt_map_label_points_device(h_, params ? params : &def, dx, dy, dz, n, pose_colmajor, d_label, &k);
    return status_ == NDT_OK ? k : 0;
  }
  // removes the components the filter rejects (filter null: ndt_map_component_filter_default_params, which removes nothing)
  ndt_map_remove_components_result mapRemoveComponents(const ndt_map_component_filter* filter,
                                                       const ndt_map_components_params* params = nullptr) {
    ndt_map_remove_components_result r{};
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return r; }
    ndt_map_components_params def;
    ndt_map_components_default_params(&def);
    ndt_map_component_filter fdef;
    ndt_map_component_filter_default_params(&fdef);
    status_ = ndt_map_remove_components(h_, params ? params : &def, filter ? filter : &fdef, &r);
    return status_ == NDT_OK ? r : ndt_map_remove_components_result{};
  }

  // box_min / box_max: three floats each, or both null for the whole map
  void mapExportState(MapState& out, const float* box_min = nullptr, const float* box_max = nullptr) {
    out = MapState{};
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    ndt_map_info mi{};
    status_ = ndt_map_get_info(h_, &mi);
    if (status_ != NDT_OK) return;
    out.leaf = mi.leaf;
    out.with_intensity = mi.with_intensity != 0;
    const bool mom = mapHasMoments();
    const size_t cap = (size_t)mi.n_voxels;   // (no selection holds more)
    out.ijk.resize(3 * cap); out.counts.resize(cap); out.sums.resize(4 * cap); out.moments.resize(mom ? 9 * cap : 0);
    size_t m = 0;
    status_ = ndt_map_export_state(h_, box_min, box_max, out.ijk.data(), out.counts.data(), out.sums.data(),
                                   mom ? out.moments.data() : nullptr, cap, &m);
    if (status_ != NDT_OK) m = 0;
    out.ijk.resize(3 * m); out.counts.resize(m); out.sums.resize(4 * m); out.moments.resize(mom ? 9 * m : 0);
  }
  void mapImportState(const MapState& s) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    const size_t n = s.counts.size();
    if (s.ijk.size() != 3 * n || s.sums.size() != 4 * n || (!s.moments.empty() && s.moments.size() != 9 * n)) {
      status_ = NDT_ERR_INVALID_ARG;
      return;
    }
    status_ = ndt_map_import_state(h_, s.leaf, s.ijk.data(), s.counts.data(), s.sums.data(),
                                   s.moments.empty() ? nullptr : s.moments.data(), n);
  }

  // ---- the map under a changed pose (ndt_map_transform, ndt_map_import_state_posed): every voxel's sums are moved as
  // the sums of its points would be and re-binned by the moved float centroid.  Pose: 16 column-major doubles, Matrix4d, or gtsam::Pose3
  // (anything with matrix()).  mapTransform returns the number of voxels afterwards. ----
  int64_t mapTransform(const double* pose_colmajor) {
    int64_t after = 0;
    status_ = h_ ? ndt_map_transform(h_, pose_colmajor, &after) : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? after : 0;
  }
  int64_t mapTransform(const Matrix4d& pose) {
    double a[16];
    detail::to_colmajor(pose, 4, 4, a);
    return mapTransform(static_cast<const double*>(a));
  }
  template <class Pose>
  auto mapTransform(const Pose& pose) -> decltype((void)pose.matrix(), int64_t()) {
    double a[16];
    detail::pose_colmajor(pose, a);
    return mapTransform(static_cast<const double*>(a));
  }
  // a state accumulated in another frame (a submap), merged under the pose that takes that frame to the map's
  void mapImportStatePosed(const MapState& s, const double* pose_colmajor) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    const size_t n = s.counts.size();
    if (s.ijk.size() != 3 * n || s.sums.size() != 4 * n || (!s.moments.empty() && s.moments.size() != 9 * n)) {
      status_ = NDT_ERR_INVALID_ARG;
      return;
    }
    status_ = ndt_map_import_state_posed(h_, s.leaf, s.ijk.data(), s.counts.data(), s.sums.data(),
                                         s.moments.empty() ? nullptr : s.moments.data(), n, pose_colmajor);
  }
  void mapImportStatePosed(const MapState& s, const Matrix4d& pose) {
    double a[16];
    detail::to_colmajor(pose, 4, 4, a);
    mapImportStatePosed(s, static_cast<const double*>(a));
  }
  template <class Pose>
  auto mapImportStatePosed(const MapState& s, const Pose& pose) -> decltype((void)pose.matrix()) {
    double a[16];
    detail::pose_colmajor(pose, a);
    mapImportStatePosed(s, static_cast<const double*>(a));
  }
  void mapImportStatePosedDevice(float leaf, const int32_t* d_ijk, const int32_t* d_count, const float* d_sums4,
                                 const double* d_moments9, size_t n, const double* pose_colmajor) {
    status_ = h_ ? ndt_map_import_state_posed_device(h_, leaf, d_ijk, d_count, d_sums4, d_moments9, n, pose_colmajor)
                 : NDT_ERR_NO_DEVICE;
  }

  // ---- levels (ndt_map_level_*, ndt_set_target_from_map_level, ndt_map_coarsen, ndt_align_map_levels): the map at
  // leaf * 2^level made from its own sums on the device, cached until the map changes; level 0 is the map itself.
  // alignMapLevels runs one align() per step, coarse to fine, each against its level as the target and from the step
  // before; the adapter's own result (getFinalTransformation, getResult) stays that of the last align(). ----
  ndt_map_info mapLevelInfo(int level) {
    ndt_map_info mi{};
    status_ = h_ ? ndt_map_level_info(h_, level, &mi) : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? mi : ndt_map_info{};
  }
  void mapExportStateLevel(int level, MapState& out, const float* box_min = nullptr, const float* box_max = nullptr) {
    out = MapState{};
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    ndt_map_info mi{};
    status_ = ndt_map_level_info(h_, level, &mi);
    if (status_ != NDT_OK) return;
    out.leaf = mi.leaf;
    out.with_intensity = mi.with_intensity != 0;
    const bool mom = mapHasMoments();
    const size_t cap = (size_t)mi.n_voxels;   // (no selection holds more)
    out.ijk.resize(3 * cap); out.counts.resize(cap); out.sums.resize(4 * cap); out.moments.resize(mom ? 9 * cap : 0);
    size_t m = 0;
    status_ = ndt_map_export_state_level(h_, level, box_min, box_max, out.ijk.data(), out.counts.data(), out.sums.data(),
                                         mom ? out.moments.data() : nullptr, cap, &m);
    if (status_ != NDT_OK) m = 0;
    out.ijk.resize(3 * m); out.counts.resize(m); out.sums.resize(4 * m); out.moments.resize(mom ? 9 * m : 0);
  }
  size_t mapExportStateLevelDevice(int level, int32_t* d_ijk, int32_t* d_count, float* d_sums4, double* d_moments9, size_t cap,
                                   const float* box_min = nullptr, const float* box_max = nullptr) {
    size_t m = 0;
    status_ = h_ ? ndt_map_export_state_level_device(h_, level, box_min, box_max, d_ijk, d_count, d_sums4, d_moments9, cap, &m)
                 : NDT_ERR_NO_DEVICE;
    return m;
  }
  void setInputTargetFromMapLevel(int level, const float* box_min = nullptr, const float* box_max = nullptr) {
    status_ = h_ ? ndt_set_target_from_map_level(h_, level, box_min, box_max) : NDT_ERR_NO_DEVICE;
  }
  void mapCoarsen(int level) { status_ = h_ ? ndt_map_coarsen(h_, level) : NDT_ERR_NO_DEVICE; }
  void mapLevelsDrop() { status_ = h_ ? ndt_map_levels_drop(h_) : NDT_ERR_NO_DEVICE; }
  // one ndt_result per step that ran (fewer than steps.size() when a step failed: lastStatus() is its code)
  std::vector<ndt_result> alignMapLevels(const std::vector<ndt_map_level_step>& steps, const Matrix4f& guess,
                                         const float* half_extent_or_null = nullptr) {
    std::vector<ndt_result> out;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return out; }
    if (steps.empty() || steps.size() > (size_t)NDT_MAP_LEVEL_STEPS_MAX) { status_ = NDT_ERR_INVALID_ARG; return out; }
    float g[16];
    detail::to_colmajor(guess, 4, 4, g);
    out.resize(steps.size());
    for (ndt_result& r : out) { std::memset(&r, 0, sizeof(r)); r.iterations = -1; }
    status_ = ndt_align_map_levels(h_, steps.data(), (int)steps.size(), half_extent_or_null, g, out.data());
    if (status_ != NDT_OK) {   // keep the steps that were written
      size_t done = 0;
      while (done < out.size() && out[done].iterations >= 0) ++done;
      out.resize(done);
    }
    return out;
  }

  // ---- distribution-to-distribution NDT (ndt_set_source_distributions, ndt_eval_derivatives_d2d, ndt_align_d2d): a
  // submap's voxels -- the counts and moments of a MapState -- registered to the target's leaves.  The distribution
  // source is separate from the point source; the adapter's own result (getFinalTransformation, getResult) stays that
  // of the last align().  The pose found is what mapImportStatePosed takes. ----
  void setInputSourceDistributions(const std::vector<int32_t>& counts, const std::vector<double>& moments) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    const size_t n = counts.size();
    if (moments.size() != 9 * n) { status_ = NDT_ERR_INVALID_ARG; return; }
    status_ = ndt_set_source_distributions(h_, n ? counts.data() : nullptr, n ? moments.data() : nullptr, n);
  }
  void setInputSourceDistributions(const MapState& s) { setInputSourceDistributions(s.counts, s.moments); }
  void setInputSourceDistributionsDevice(const int32_t* d_count, const double* d_moments9, size_t n) {
    status_ = h_ ? ndt_set_source_distributions_device(h_, d_count, d_moments9, n) : NDT_ERR_NO_DEVICE;
  }
  // the accepted source Gaussians in input order
  struct SourceDistributions {
    std::vector<double> mean;            // 3 per Gaussian
    std::vector<double> cov;             // 6 per Gaussian: xx, xy, xz, yy, yz, zz
    std::vector<int32_t> counts, record_index;
    int64_t n_records = 0;               // records handed over, the rejected ones included
    size_t size() const { return counts.size(); }
  };
  SourceDistributions getSourceDistributions() {
    SourceDistributions out;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return out; }
    int64_t n_acc = 0;
    status_ = ndt_source_distributions_info(h_, &out.n_records, &n_acc);
    if (status_ != NDT_OK || n_acc <= 0) return out;
    const size_t m = (size_t)n_acc;
    out.mean.resize(3 * m); out.cov.resize(6 * m); out.counts.resize(m); out.record_index.resize(m);
    const int64_t got = ndt_export_source_distributions(h_, out.mean.data(), out.cov.data(), out.counts.data(),
                                                        out.record_index.data(), m);
    if (got != n_acc) { status_ = got < 0 ? (int)got : NDT_ERR_INVALID_ARG; out = SourceDistributions(); }
    return out;
  }
  // score, gradient and Hessian of the D2D objective at p = [x, y, z, roll, pitch, yaw] (one launch)
  template <class Vec6, class Mat6>
  double computeDerivativesD2D(Vec6& score_gradient, Mat6& hessian, const Vec6& p, bool compute_hessian = true) {
    double pose[6], words[NDT_EVAL_WORDS], score = 0.0, g[6], H[36];
    for (int i = 0; i < 6; ++i) { pose[i] = p[i]; score_gradient[i] = 0.0; }
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) hessian(r, c) = 0.0;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return 0.0; }
    status_ = ndt_eval_derivatives_d2d(h_, pose, 1, compute_hessian ? 1 : 0, words);
    if (status_ != NDT_OK) return 0.0;
    ndt_unpack_eval(words, &score, g, H);
    for (int i = 0; i < 6; ++i) score_gradient[i] = g[i];
    if (compute_hessian)
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) hessian(r, c) = H[6 * r + c];
    return score;
  }
  // the result as alignMany gives one: `pose` takes the submap's frame to the target's; on an error it holds the guess.
  // converged_or_null receives ndt_result::converged.
  NdtResult alignDistributions(const Matrix4f& guess, bool* converged_or_null = nullptr) {
    float g[16];
    detail::to_colmajor(guess, 4, 4, g);
    ndt_result raw;
    std::memset(&raw, 0, sizeof(raw));
    status_ = h_ ? ndt_align_d2d(h_, g, &raw) : NDT_ERR_NO_DEVICE;
    if (status_ != NDT_OK) {
      std::memset(&raw, 0, sizeof(raw));
      std::memcpy(raw.final_transformation, g, sizeof(g));
    }
    if (converged_or_null) *converged_or_null = raw.converged != 0;
    NdtResult out;
    out.pose = detail::from_colmajor<Matrix4f>(raw.final_transformation, 4, 4);
    out.transform_probability = (float)raw.transform_probability;
    out.nearest_voxel_transformation_likelihood = (float)raw.nearest_voxel_transformation_likelihood;
    out.iteration_num = raw.iterations;
    out.hessian = detail::from_rowmajor<Matrix6d>(raw.hessian, 6, 6);
    return out;
  }

  // ---- continuous-time NDT (ndt_set_source_times, ndt_eval_derivatives_ct, ndt_align_ct, ndt_transform_source_ct): a scan
  // captured in motion, every point with its own pose between the scan's begin pose (the previous scan's end pose) and
  // the end pose being estimated.  The times are PCLPointCloud::pointsAlpha, one per point of the input source, set AFTER
  // setInputSource (every source setter drops them).  `begin` is [x, y, z, roll, pitch, yaw] or a 4 x 4 -- a previous
  // getFinalTransformation() or ContinuousTimeResult::pose can be passed straight in.  Any Euler triple of the begin
  // rotation serves, in every call below: the engine fits the begin pose's angles to the branch of the end pose's (of the
  // guess's, in the align) before it blends -- THE FIT of ndt_hip.h -- so poseOfMatrix need not be, and is not, the
  // engine's own matrix-to-pose conversion (whose roll lies in [0, pi]).  The adapter's own result
  // (getFinalTransformation, getResult) stays that of the last align(). ----
  using Pose6 = std::array<double, 6>;
  template <class Mat4>
  static Pose6 poseOfMatrix(const Mat4& T) {   // the angles of R = Rx Ry Rz, pitch in [-pi/2, pi/2]
    Pose6 p;
    p[0] = T(0, 3); p[1] = T(1, 3); p[2] = T(2, 3);
    p[3] = std::atan2(-(double)T(1, 2), (double)T(2, 2));
    p[4] = std::atan2((double)T(0, 2), std::sqrt((double)T(0, 0) * (double)T(0, 0) + (double)T(0, 1) * (double)T(0, 1)));
    p[5] = std::atan2(-(double)T(0, 1), (double)T(0, 0));
    return p;
  }
  void setInputSourceTimes(const float* alpha, size_t n) { status_ = h_ ? ndt_set_source_times(h_, alpha, n) : NDT_ERR_NO_DEVICE; }
  void setInputSourceTimes(const std::vector<float>& alpha) { setInputSourceTimes(alpha.empty() ? nullptr : alpha.data(), alpha.size()); }
  int64_t sourceTimesCount() const { return h_ ? ndt_source_times_info(h_) : 0; }
  // score, gradient and Hessian of the continuous-time objective at the END pose p (one launch)
  template <class Vec6, class Mat6>
  double computeDerivativesCT(Vec6& score_gradient, Mat6& hessian, const Pose6& begin, const Vec6& p, bool compute_hessian = true) {
    double pose[6], words[NDT_EVAL_WORDS], score = 0.0, g[6], H[36];
    for (int i = 0; i < 6; ++i) { pose[i] = p[i]; score_gradient[i] = 0.0; }
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) hessian(r, c) = 0.0;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return 0.0; }
    status_ = ndt_eval_derivatives_ct(h_, begin.data(), pose, 1, compute_hessian ? 1 : 0, words);
    if (status_ != NDT_OK) return 0.0;
    ndt_unpack_eval(words, &score, g, H);
    for (int i = 0; i < 6; ++i) score_gradient[i] = g[i];
    if (compute_hessian)
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) hessian(r, c) = H[6 * r + c];
    return score;
  }
  template <class Vec6, class Mat6>
  double computeDerivativesCT(Vec6& score_gradient, Mat6& hessian, const Matrix4f& begin, const Vec6& p, bool compute_hessian = true) {
    return computeDerivativesCT(score_gradient, hessian, poseOfMatrix(begin), p, compute_hessian);
  }
  // the result as alignDistributions gives one, with the end pose as six numbers -- the next scan's `begin`; on an error
  // `pose` holds the guess and end_pose its angles
  struct ContinuousTimeResult : NdtResult {
    Pose6 end_pose{};
    bool converged = false;
  };
  ContinuousTimeResult alignContinuousTime(const Pose6& begin, const Matrix4f& guess) {
    float g[16];
    detail::to_colmajor(guess, 4, 4, g);
    ndt_result raw;
    std::memset(&raw, 0, sizeof(raw));
    status_ = h_ ? ndt_align_ct(h_, begin.data(), g, &raw) : NDT_ERR_NO_DEVICE;
    ContinuousTimeResult out;
    if (status_ != NDT_OK) {
      std::memset(&raw, 0, sizeof(raw));
      std::memcpy(raw.final_transformation, g, sizeof(g));
      out.end_pose = poseOfMatrix(guess);
    } else {
      for (int i = 0; i < 6; ++i) out.end_pose[i] = raw.final_pose[i];
    }
    out.converged = raw.converged != 0;
    out.pose = detail::from_colmajor<Matrix4f>(raw.final_transformation, 4, 4);
    out.transform_probability = (float)raw.transform_probability;
    out.nearest_voxel_transformation_likelihood = (float)raw.nearest_voxel_transformation_likelihood;
    out.iteration_num = raw.iterations;
    out.hessian = detail::from_rowmajor<Matrix6d>(raw.hessian, 6, 6);
    return out;
  }
  ContinuousTimeResult alignContinuousTime(const Matrix4f& begin, const Matrix4f& guess) {
    return alignContinuousTime(poseOfMatrix(begin), guess);
  }
  // the deskewed scan under begin and end pose: frame 0 in the end pose's frame (what putKeyframe / mapAdd take with the
  // result), frame 1 in the target's frame; out.points[i] belongs to source point i (NaN for a non-finite point or time).
  // On error: an empty cloud, lastStatus() says why.
  template <class Cloud>
  void getDeskewedSource(const Pose6& begin, const Pose6& end, Cloud& out, int frame = 0) {
    out.points.clear();
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    const int64_t n = ndt_source_size(h_);
    if (n < 0) { status_ = (int)n; return; }
    std::vector<float> xyz(3 * (size_t)n + 3);
    status_ = ndt_transform_source_ct(h_, begin.data(), end.data(), frame, xyz.data(), (size_t)n);
    if (status_ != NDT_OK) return;
    out.points.resize((size_t)n);   // value-initialised points: the fields the engine does not write keep their defaults
    for (size_t i = 0; i < (size_t)n; ++i) {
      out.points[i].x = xyz[3 * i];
      out.points[i].y = xyz[3 * i + 1];
      out.points[i].z = xyz[3 * i + 2];
    }
  }
  template <class Cloud>
  void getDeskewedSource(const Matrix4f& begin, const Pose6& end, Cloud& out, int frame = 0) {
    getDeskewedSource(poseOfMatrix(begin), end, out, frame);
  }

  // ---- device-resident keyframe archive (ref: run/pipeline_ligo_tc.cpp:519-529, run/pipeline.cpp:554-557,784) ----
  // not part of pclomp: the body-frame scans stay in HBM, the sliding-window target is assembled
  // there from ids + poses (column-major 4x4 doubles, e.g. gtsam::Pose3::matrix().data())
  template <class Cloud>
  void putKeyframe(int64_t id, const Cloud& cloud) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    status_ = cloud.points.empty() ? ndt_keyframe_put(h_, id, nullptr, 0, 12)
                                   : ndt_keyframe_put(h_, id, &cloud.points[0].x, cloud.points.size(), sizeof(cloud.points[0]));
  }
  void eraseKeyframe(int64_t id) { status_ = h_ ? ndt_keyframe_erase(h_, id) : NDT_ERR_NO_DEVICE; }
  int64_t keyframeCount() const { return h_ ? ndt_keyframe_count(h_) : 0; }
  // poses_colmajor: ids.size() x 16 doubles
  void setInputTargetFromKeyframes(const std::vector<int64_t>& ids, const double* poses_colmajor) {
    status_ = h_ ? ndt_set_target_from_keyframes(h_, ids.data(), poses_colmajor, (int)ids.size()) : NDT_ERR_NO_DEVICE;
  }
  void setInputSourceFromKeyframe(int64_t id) {
    status_ = h_ ? ndt_set_source_from_keyframe(h_, id) : NDT_ERR_NO_DEVICE;
    if (status_ == NDT_OK) n_src_ = 0;  // align()'s output cloud is not filled on this path
  }

  // ---- Scan Context place recognition over the keyframe archive (ndt_scan_context* in ndt_hip.h): a scan's
  // rings x sectors descriptor of maximum heights, the descriptor bank beside the archive, and the match of one query with
  // every entry at every column shift.  Not part of pclomp.  A descriptor is n_rings * n_sectors floats, row = ring. ----
  void setScanContextParams(const ndt_scan_context_params& p) {   // a change clears the bank
    status_ = h_ ? ndt_scan_context_set_params(h_, &p) : NDT_ERR_NO_DEVICE;
  }
  ndt_scan_context_params getScanContextParams() {
    ndt_scan_context_params p;
    ndt_scan_context_default_params(&p);
    status_ = h_ ? ndt_scan_context_get_params(h_, &p) : NDT_ERR_NO_DEVICE;
    return p;
  }
  // the descriptor of a cloud in the sensor's frame; counts_or_null receives the points per bin.  Empty on error.
  template <class Cloud>
  std::vector<float> scanContext(const Cloud& cloud, std::vector<int32_t>* counts_or_null = nullptr) {
    std::vector<float> desc;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return desc; }
    const ndt_scan_context_params p = getScanContextParams();
    if (status_ != NDT_OK) return desc;
    const size_t bins = (size_t)p.n_rings * (size_t)p.n_sectors;
    desc.assign(bins, 0.0f);
    if (counts_or_null) counts_or_null->assign(bins, 0);
    int32_t* cnt = counts_or_null ? counts_or_null->data() : nullptr;
    status_ = cloud.points.empty()
                  ? ndt_scan_context(h_, nullptr, 0, 12, desc.data(), cnt)
                  : ndt_scan_context(h_, &cloud.points[0].x, cloud.points.size(), sizeof(cloud.points[0]), desc.data(), cnt);
    if (status_ != NDT_OK) desc.clear();
    return desc;
  }
  // device arrays in, device memory of n_rings * n_sectors words out (d_count may be null)
  void scanContextDevice(const float* dx, const float* dy, const float* dz, size_t n, float* d_desc, int32_t* d_count = nullptr) {
    status_ = h_ ? ndt_scan_context_device(h_, dx, dy, dz, n, d_desc, d_count) : NDT_ERR_NO_DEVICE;
  }
  // the archived scan `id`: its descriptor goes into the bank under the same id and comes back
  std::vector<float> scanContextKeyframe(int64_t id, std::vector<int32_t>* counts_or_null = nullptr) {
    std::vector<float> desc;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return desc; }
    const ndt_scan_context_params p = getScanContextParams();
    if (status_ != NDT_OK) return desc;
    const size_t bins = (size_t)p.n_rings * (size_t)p.n_sectors;
    desc.assign(bins, 0.0f);
    if (counts_or_null) counts_or_null->assign(bins, 0);
    status_ = ndt_scan_context_keyframe(h_, id, desc.data(), counts_or_null ? counts_or_null->data() : nullptr);
    if (status_ != NDT_OK) desc.clear();
    return desc;
  }
  void scanContextBankPut(int64_t id, const std::vector<float>& desc) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    const ndt_scan_context_params p = getScanContextParams();
    if (status_ != NDT_OK) return;
    if (desc.size() != (size_t)p.n_rings * (size_t)p.n_sectors) { status_ = NDT_ERR_INVALID_ARG; return; }
    status_ = ndt_scan_context_bank_put(h_, id, desc.data());
  }
  std::vector<float> scanContextBankGet(int64_t id) {
    std::vector<float> desc;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return desc; }
    const ndt_scan_context_params p = getScanContextParams();
    if (status_ != NDT_OK) return desc;
    desc.assign((size_t)p.n_rings * (size_t)p.n_sectors, 0.0f);
    status_ = ndt_scan_context_bank_get(h_, id, desc.data());
    if (status_ != NDT_OK) desc.clear();
    return desc;
  }
  void scanContextBankErase(int64_t id) { status_ = h_ ? ndt_scan_context_bank_erase(h_, id) : NDT_ERR_NO_DEVICE; }
  void scanContextBankClear() { status_ = h_ ? ndt_scan_context_bank_clear(h_) : NDT_ERR_NO_DEVICE; }
  int64_t scanContextBankCount() const { return h_ ? ndt_scan_context_bank_count(h_) : 0; }
  // one element per bank entry, ascending ids; best(): the entry of least distance (-1: the bank is empty)
  struct ScanContextMatches {
    std::vector<int64_t> ids;
    std::vector<double> distance;
    std::vector<int32_t> shift, columns;
    size_t size() const { return ids.size(); }
    long best() const {
      long at = -1;
      for (size_t i = 0; i < distance.size(); ++i)
        if (at < 0 || distance[i] < distance[(size_t)at]) at = (long)i;
      return at;
    }
  };
  ScanContextMatches scanContextMatch(const std::vector<float>& desc) {
    ScanContextMatches out;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return out; }
    const ndt_scan_context_params p = getScanContextParams();
    if (status_ != NDT_OK) return out;
    if (desc.size() != (size_t)p.n_rings * (size_t)p.n_sectors) { status_ = NDT_ERR_INVALID_ARG; return out; }
    return scan_context_matches_(true, desc.data(), 0);
  }
  // the query is the bank entry `id`, read on the device; it is among the results
  ScanContextMatches scanContextMatchKeyframe(int64_t id) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return ScanContextMatches(); }
    return scan_context_matches_(false, nullptr, id);
  }
  // yaw = shift * 2 pi / n_sectors wrapped to (-pi, pi]: Rz(yaw) is the guess that aligns the query scan to the candidate
  static double scanContextYaw(int shift, int n_sectors) {
    const double two_pi = 6.283185307179586476925286766559;
    return (double)(2 * shift > n_sectors ? shift - n_sectors : shift) * (two_pi / (double)n_sectors);
  }

  // ---- deskew: a scan expressed in one pose, from per-point times and a pose trajectory (ndt_deskew* in ndt_hip.h:
  // position blended linearly, attitude by slerp, times clamped to the knots; ref_pose null = the last knot), with the
  // acquisition filter of the lidar callback in the same pass (filter null: every point comes back, a non-finite one
  // as NaN).  Not part of pclomp -- the reference computes pointsAlpha and never reads it.  Each returns the number of
  // points written / archived (0 on error, lastStatus() says why). ----
  size_t deskew(const float* xyz, size_t n, size_t stride_bytes, long intensity_offset_bytes, const float* t,
                const double* knot_t, const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
                const ndt_scan_filter* filter_or_null, float* out, int32_t* index_out, size_t cap) {
    size_t m = 0;
    status_ = h_ ? ndt_deskew(h_, xyz, n, stride_bytes, intensity_offset_bytes, t, knot_t, knot_poses16, n_knots,
                              ref_pose16_or_null, filter_or_null, out, index_out, cap, &m)
                 : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? m : 0;
  }
  size_t deskewDevice(const float* dx, const float* dy, const float* dz, const float* d_intensity, const float* d_t, size_t n,
                      const double* knot_t, const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
                      const ndt_scan_filter* filter_or_null, float* ox, float* oy, float* oz, float* o_intensity,
                      int32_t* d_index_out, size_t cap) {
    size_t m = 0;
    status_ = h_ ? ndt_deskew_device(h_, dx, dy, dz, d_intensity, d_t, n, knot_t, knot_poses16, n_knots, ref_pose16_or_null,
                                     filter_or_null, ox, oy, oz, o_intensity, d_index_out, cap, &m)
                 : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? m : 0;
  }
  // archives the deskewed scan under `id` (one upload serves the archive and, through setInputSourceFromKeyframe, the
  // source); the frame's pose is then the reference pose
  size_t putKeyframeDeskewed(int64_t id, const float* xyz, size_t n, size_t stride_bytes, long intensity_offset_bytes,
                             const float* t, const double* knot_t, const double* knot_poses16, int n_knots,
                             const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null) {
    size_t m = 0;
    status_ = h_ ? ndt_keyframe_put_deskewed(h_, id, xyz, n, stride_bytes, intensity_offset_bytes, t, knot_t, knot_poses16,
                                             n_knots, ref_pose16_or_null, filter_or_null, &m)
                 : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? m : 0;
  }
  // the typed face: a cloud (pcl::PointCloud<pcl::PointXYZI>: the intensity travels and feeds the filter), one time per
  // point, the knots' times and poses (std::vector<Eigen::Matrix4d>, or any indexable container of 4 x 4 matrices)
  template <class Cloud, class Poses>
  Cloud deskew(const Cloud& scan, const std::vector<float>& t, const std::vector<double>& knot_t, const Poses& knot_poses,
               const Matrix4d* ref_pose = nullptr, const ndt_scan_filter* filter = nullptr, std::vector<int32_t>* index = nullptr) {
    Cloud out;
    if (index) index->clear();
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return out; }
    if (t.size() != scan.points.size() || knot_t.size() != knot_poses.size()) { status_ = NDT_ERR_INVALID_ARG; return out; }
    using P = typename std::decay<decltype(scan.points[0])>::type;
    const size_t n = scan.points.size();
    const std::vector<double> poses = detail::pack_poses(knot_poses);
    double ref[16];
    if (ref_pose) detail::to_colmajor(*ref_pose, 4, 4, ref);
    out.points.resize(n);   // value-initialised points: the fields the engine does not write keep their defaults
    std::vector<int32_t> idx(index ? n + 1 : 0);
    const size_t m = deskew(n ? &scan.points[0].x : nullptr, n, sizeof(P), intensity_offset_of<P>(0), t.data(), knot_t.data(),
                            poses.data(), (int)knot_t.size(), ref_pose ? ref : nullptr, filter, n ? &out.points[0].x : nullptr,
                            index ? idx.data() : nullptr, n);
    out.points.resize(m);
    if (index && status_ == NDT_OK) index->assign(idx.begin(), idx.begin() + (std::ptrdiff_t)m);
    return out;
  }
  template <class Cloud, class Poses>
  size_t putKeyframeDeskewed(int64_t id, const Cloud& scan, const std::vector<float>& t, const std::vector<double>& knot_t,
                             const Poses& knot_poses, const Matrix4d* ref_pose = nullptr, const ndt_scan_filter* filter = nullptr) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return 0; }
    if (t.size() != scan.points.size() || knot_t.size() != knot_poses.size()) { status_ = NDT_ERR_INVALID_ARG; return 0; }
    using P = typename std::decay<decltype(scan.points[0])>::type;
    const size_t n = scan.points.size();
    const std::vector<double> poses = detail::pack_poses(knot_poses);
    double ref[16];
    if (ref_pose) detail::to_colmajor(*ref_pose, 4, 4, ref);
    return putKeyframeDeskewed(id, n ? &scan.points[0].x : nullptr, n, sizeof(P), intensity_offset_of<P>(0), t.data(),
                               knot_t.data(), poses.data(), (int)knot_t.size(), ref_pose ? ref : nullptr, filter);
  }
  // ---- unprojection: the lidar callback's range image (a 20-bit range in millimetres and a reflectivity byte per pixel,
  // one time per column, column by column) through the scan model's tables to points, with the range gate, the
  // acquisition filter and the deskew in the same pass (ndt_unproject* in ndt_hip.h).  Replaces the point-forming part
  // of LidarCallback::DecodePacket*; packet parsing stays with the driver (or goes to the device too: pushPackets below). ----
  // the tables as the callback's Initialize() computes them (host only); x1 .. z1: n_cols * n_rows, x2 .. z2: n_cols
  struct ScanModel {
    int n_cols = 0, n_rows = 0;
    std::vector<float> x1, y1, z1, x2, y2, z2;
  };
  static bool scanModelFromBeams(int n_cols, const std::vector<float>& beam_azimuth_deg, const std::vector<float>& beam_altitude_deg,
                                 double lidar_origin_to_beam_origin_mm, const Matrix4d* lidar_to_body, ScanModel& out) {
    if (n_cols < 1 || beam_azimuth_deg.empty() || beam_azimuth_deg.size() != beam_altitude_deg.size()) return false;
    const int n_rows = (int)beam_azimuth_deg.size();
    const size_t n = (size_t)n_cols * (size_t)n_rows;
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (lidar_to_body) detail::to_colmajor(*lidar_to_body, 4, 4, T);
    ScanModel m;
    m.n_cols = n_cols; m.n_rows = n_rows;
    m.x1.resize(n); m.y1.resize(n); m.z1.resize(n);
    m.x2.resize((size_t)n_cols); m.y2.resize((size_t)n_cols); m.z2.resize((size_t)n_cols);
    if (ndt_scan_model_from_beams(n_cols, n_rows, beam_azimuth_deg.data(), beam_altitude_deg.data(), lidar_origin_to_beam_origin_mm, T,
                                  m.x1.data(), m.y1.data(), m.z1.data(), m.x2.data(), m.y2.data(), m.z2.data()) != NDT_OK)
      return false;
    out = std::move(m);
    return true;
  }
  void setScanModel(int n_cols, int n_rows, const float* x1, const float* y1, const float* z1, const float* x2, const float* y2,
                    const float* z2) {
    status_ = h_ ? ndt_scan_model_set(h_, n_cols, n_rows, x1, y1, z1, x2, y2, z2) : NDT_ERR_NO_DEVICE;
  }
  void setScanModel(const ScanModel& m) {
    const size_t n = (size_t)m.n_cols * (size_t)m.n_rows, nc = (size_t)m.n_cols;
    if (m.n_cols < 1 || m.n_rows < 1 || m.x1.size() != n || m.y1.size() != n || m.z1.size() != n || m.x2.size() != nc ||
        m.y2.size() != nc || m.z2.size() != nc) {
      status_ = NDT_ERR_INVALID_ARG;
      return;
    }
    setScanModel(m.n_cols, m.n_rows, m.x1.data(), m.y1.data(), m.z1.data(), m.x2.data(), m.y2.data(), m.z2.data());
  }
  void clearScanModel() { status_ = h_ ? ndt_scan_model_clear(h_) : NDT_ERR_NO_DEVICE; }
  // pixels of the scan model that is set (0: none)
  size_t scanModelPixels(int* n_cols = nullptr, int* n_rows = nullptr) const {
    int c = 0, r = 0;
    if (h_) (void)ndt_scan_model_get_info(h_, &c, &r);
    if (n_cols) *n_cols = c;
    if (n_rows) *n_rows = r;
    return (size_t)c * (size_t)r;
  }
  // each returns the number of points written / archived (0 on error, lastStatus() says why); n_knots == 0 with the three
  // trajectory pointers null: no motion
  size_t unproject(const uint32_t* range_mm, const uint8_t* reflectivity, const float* col_t, const ndt_range_gate* gate_or_null,
                   const double* knot_t, const double* knot_poses16, int n_knots, const double* ref_pose16_or_null,
                   const ndt_scan_filter* filter_or_null, float* out, size_t stride_bytes, long intensity_offset_bytes, float* t_out,
                   int32_t* index_out, size_t cap) {
    size_t m = 0;
    status_ = h_ ? ndt_unproject(h_, range_mm, reflectivity, col_t, gate_or_null, knot_t, knot_poses16, n_knots, ref_pose16_or_null,
                                 filter_or_null, out, stride_bytes, intensity_offset_bytes, t_out, index_out, cap, &m)
                 : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? m : 0;
  }
  size_t unprojectDevice(const uint32_t* d_range_mm, const uint8_t* d_reflectivity, const float* d_col_t,
                         const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16, int n_knots,
                         const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* ox, float* oy, float* oz,
                         float* o_intensity, float* o_t, int32_t* d_index_out, size_t cap) {
    size_t m = 0;
    status_ = h_ ? ndt_unproject_device(h_, d_range_mm, d_reflectivity, d_col_t, gate_or_null, knot_t, knot_poses16, n_knots,
                                        ref_pose16_or_null, filter_or_null, ox, oy, oz, o_intensity, o_t, d_index_out, cap, &m)
                 : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? m : 0;
  }
  size_t putKeyframeFromRanges(int64_t id, const uint32_t* range_mm, const uint8_t* reflectivity, const float* col_t,
                               const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16, int n_knots,
                               const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null) {
    size_t m = 0;
    status_ = h_ ? ndt_keyframe_put_from_ranges(h_, id, range_mm, reflectivity, col_t, gate_or_null, knot_t, knot_poses16, n_knots,
                                                ref_pose16_or_null, filter_or_null, &m)
                 : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? m : 0;
  }
  // the typed face: the range image as vectors (n_cols * n_rows ranges and reflectivities -- the latter may be empty --,
  // n_cols times), the knots' times and poses (both empty: no motion); returns the cloud (filter null: organised, every
  // pixel, an invalid one as NaN) and, if asked for, each point's time and pixel index
  template <class Cloud, class Poses>
  Cloud unproject(const std::vector<uint32_t>& range_mm, const std::vector<uint8_t>& reflectivity, const std::vector<float>& col_t,
                  const std::vector<double>& knot_t, const Poses& knot_poses, const Matrix4d* ref_pose = nullptr,
                  const ndt_range_gate* gate = nullptr, const ndt_scan_filter* filter = nullptr, std::vector<float>* times = nullptr,
                  std::vector<int32_t>* index = nullptr) {
    Cloud out;
    if (times) times->clear();
    if (index) index->clear();
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return out; }
    int n_cols = 0;
    const size_t n = scanModelPixels(&n_cols);
    if (range_mm.size() != n || col_t.size() != (size_t)n_cols || (!reflectivity.empty() && reflectivity.size() != n) ||
        knot_t.size() != knot_poses.size()) {
      status_ = NDT_ERR_INVALID_ARG;
      return out;
    }
    using P = typename std::decay<decltype(out.points[0])>::type;
    const bool moving = !knot_t.empty();
    const std::vector<double> poses = detail::pack_poses(knot_poses);
    double ref[16];
    if (ref_pose) detail::to_colmajor(*ref_pose, 4, 4, ref);
    out.points.resize(n);   // value-initialised points: the fields the engine does not write keep their defaults
    std::vector<float> tt(times ? n + 1 : 0);
    std::vector<int32_t> idx(index ? n + 1 : 0);
    const size_t m = unproject(range_mm.data(), reflectivity.empty() ? nullptr : reflectivity.data(), col_t.data(), gate,
                               moving ? knot_t.data() : nullptr, moving ? poses.data() : nullptr, (int)knot_t.size(),
                               ref_pose ? ref : nullptr, filter, n ? &out.points[0].x : nullptr, sizeof(P),
                               reflectivity.empty() ? -1 : intensity_offset_of<P>(0), times ? tt.data() : nullptr,
                               index ? idx.data() : nullptr, n);
    out.points.resize(m);
    if (times && status_ == NDT_OK) times->assign(tt.begin(), tt.begin() + (std::ptrdiff_t)m);
    if (index && status_ == NDT_OK) index->assign(idx.begin(), idx.begin() + (std::ptrdiff_t)m);
    return out;
  }
  template <class Poses>
  size_t putKeyframeFromRanges(int64_t id, const std::vector<uint32_t>& range_mm, const std::vector<uint8_t>& reflectivity,
                               const std::vector<float>& col_t, const std::vector<double>& knot_t, const Poses& knot_poses,
                               const Matrix4d* ref_pose = nullptr, const ndt_range_gate* gate = nullptr,
                               const ndt_scan_filter* filter = nullptr) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return 0; }
    int n_cols = 0;
    const size_t n = scanModelPixels(&n_cols);
    if (range_mm.size() != n || col_t.size() != (size_t)n_cols || (!reflectivity.empty() && reflectivity.size() != n) ||
        knot_t.size() != knot_poses.size()) {
      status_ = NDT_ERR_INVALID_ARG;
      return 0;
    }
    const bool moving = !knot_t.empty();
    const std::vector<double> poses = detail::pack_poses(knot_poses);
    double ref[16];
    if (ref_pose) detail::to_colmajor(*ref_pose, 4, 4, ref);
    return putKeyframeFromRanges(id, range_mm.data(), reflectivity.empty() ? nullptr : reflectivity.data(), col_t.data(), gate,
                                 moving ? knot_t.data() : nullptr, moving ? poses.data() : nullptr, (int)knot_t.size(),
                                 ref_pose ? ref : nullptr, filter);
  }
  // ---- lidar packets: the UDP payloads of a frame (the lidar callback's DataBuffer) decoded on the device, then the calls
  // above on the decoded image (ndt_packet_* / ndt_unproject_packet_frame* in ndt_hip.h).  Replaces the whole of
  // LidarCallback::DecodePacket*: the host reads the column headers, a kernel gathers the pixels. ----
  void setPacketFormat(int profile, int columns_per_packet) {
    status_ = h_ ? ndt_packet_format_set(h_, profile, columns_per_packet) : NDT_ERR_NO_DEVICE;
  }
  size_t packetSize() const { return h_ ? ndt_packet_size(h_) : 0; }
  void beginPacketFrame() { status_ = h_ ? ndt_packet_frame_begin(h_) : NDT_ERR_NO_DEVICE; }
  // each returns the number of packets taken; fewer than given: a packet of the next frame stopped the call
  // (packetFrameInfo().next_frame_pending) -- finish the frame, beginPacketFrame(), push the rest
  size_t pushPackets(const uint8_t* packets, const size_t* bytes_each, size_t n_packets, size_t stride_bytes) {
    size_t taken = 0;
    status_ = h_ ? ndt_packet_frame_push(h_, packets, bytes_each, n_packets, stride_bytes, &taken) : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? taken : 0;
  }
  size_t pushPackets(const std::vector<uint8_t>& packet) {
    const size_t bytes = packet.size();
    return pushPackets(packet.data(), &bytes, 1, bytes);
  }
  size_t pushPackets(const std::vector<std::vector<uint8_t>>& packets) {
    size_t taken = 0;
    for (const std::vector<uint8_t>& p : packets) {
      if (pushPackets(p) != 1) break;
      ++taken;
    }
    return taken;
  }
  ndt_packet_frame_info packetFrameInfo() const {
    ndt_packet_frame_info info;
    std::memset(&info, 0, sizeof(info));
    info.frame_id = -1;
    if (h_) (void)ndt_packet_frame_get_info(h_, &info);
    return info;
  }
  void decodePacketFrameDevice(uint32_t* d_range_mm, uint8_t* d_reflectivity, uint16_t* d_signal, uint16_t* d_nir, float* d_col_t) {
    status_ = h_ ? ndt_decode_packet_frame_device(h_, d_range_mm, d_reflectivity, d_signal, d_nir, d_col_t) : NDT_ERR_NO_DEVICE;
  }
  size_t unprojectPacketFrameDevice(const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16, int n_knots,
                                    const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* ox, float* oy,
                                    float* oz, float* o_intensity, float* o_t, int32_t* d_index_out, uint16_t* d_signal_out,
                                    uint16_t* d_nir_out, size_t cap) {
    size_t m = 0;
    status_ = h_ ? ndt_unproject_packet_frame_device(h_, gate_or_null, knot_t, knot_poses16, n_knots, ref_pose16_or_null, filter_or_null,
                                                     ox, oy, oz, o_intensity, o_t, d_index_out, d_signal_out, d_nir_out, cap, &m)
                 : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? m : 0;
  }
  size_t unprojectPacketFrame(const ndt_range_gate* gate_or_null, const double* knot_t, const double* knot_poses16, int n_knots,
                              const double* ref_pose16_or_null, const ndt_scan_filter* filter_or_null, float* out, size_t stride_bytes,
                              long intensity_offset_bytes, float* t_out, int32_t* index_out, uint16_t* signal_out, uint16_t* nir_out,
                              size_t cap) {
    size_t m = 0;
    status_ = h_ ? ndt_unproject_packet_frame(h_, gate_or_null, knot_t, knot_poses16, n_knots, ref_pose16_or_null, filter_or_null, out,
                                              stride_bytes, intensity_offset_bytes, t_out, index_out, signal_out, nir_out, cap, &m)
                 : NDT_ERR_NO_DEVICE;
    return status_ == NDT_OK ? m : 0;
  }
  // the typed face, as unproject<Cloud>() above: the cloud of the frame in progress and, if asked for, each point's time,
  // pixel index, signal and nir
  template <class Cloud, class Poses>
  Cloud unprojectPacketFrame(const std::vector<double>& knot_t, const Poses& knot_poses, const Matrix4d* ref_pose = nullptr,
                             const ndt_range_gate* gate = nullptr, const ndt_scan_filter* filter = nullptr,
                             std::vector<float>* times = nullptr, std::vector<int32_t>* index = nullptr,
                             std::vector<uint16_t>* signal = nullptr, std::vector<uint16_t>* nir = nullptr) {
    Cloud out;
    if (times) times->clear();
    if (index) index->clear();
    if (signal) signal->clear();
    if (nir) nir->clear();
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return out; }
    if (knot_t.size() != knot_poses.size()) { status_ = NDT_ERR_INVALID_ARG; return out; }
    const size_t n = scanModelPixels();
    using P = typename std::decay<decltype(out.points[0])>::type;
    const bool moving = !knot_t.empty();
    const std::vector<double> poses = detail::pack_poses(knot_poses);
    double ref[16];
    if (ref_pose) detail::to_colmajor(*ref_pose, 4, 4, ref);
    out.points.resize(n);
    std::vector<float> tt(times ? n + 1 : 0);
    std::vector<int32_t> idx(index ? n + 1 : 0);
    std::vector<uint16_t> sg(signal ? n + 1 : 0), nr(nir ? n + 1 : 0);
    const size_t m = unprojectPacketFrame(gate, moving ? knot_t.data() : nullptr, moving ? poses.data() : nullptr, (int)knot_t.size(),
                                          ref_pose ? ref : nullptr, filter, n ? &out.points[0].x : nullptr, sizeof(P),
                                          intensity_offset_of<P>(0), times ? tt.data() : nullptr, index ? idx.data() : nullptr,
                                          signal ? sg.data() : nullptr, nir ? nr.data() : nullptr, n);
    out.points.resize(m);
    if (status_ != NDT_OK) return out;
    if (times) times->assign(tt.begin(), tt.begin() + (std::ptrdiff_t)m);
    if (index) index->assign(idx.begin(), idx.begin() + (std::ptrdiff_t)m);
    if (signal) signal->assign(sg.begin(), sg.begin() + (std::ptrdiff_t)m);
    if (nir) nir->assign(nr.begin(), nr.begin() + (std::ptrdiff_t)m);
    return out;
  }
  template <class Poses>
  size_t putKeyframeFromPackets(int64_t id, const std::vector<double>& knot_t, const Poses& knot_poses, const Matrix4d* ref_pose = nullptr,
                                const ndt_range_gate* gate = nullptr, const ndt_scan_filter* filter = nullptr,
                                std::vector<uint16_t>* signal = nullptr, std::vector<uint16_t>* nir = nullptr) {
    if (signal) signal->clear();
    if (nir) nir->clear();
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return 0; }
    if (knot_t.size() != knot_poses.size()) { status_ = NDT_ERR_INVALID_ARG; return 0; }
    const size_t n = scanModelPixels();
    const bool moving = !knot_t.empty();
    const std::vector<double> poses = detail::pack_poses(knot_poses);
    double ref[16];
    if (ref_pose) detail::to_colmajor(*ref_pose, 4, 4, ref);
    std::vector<uint16_t> sg(signal ? n + 1 : 0), nr(nir ? n + 1 : 0);
    size_t m = 0;
    status_ = ndt_keyframe_put_from_packets(h_, id, gate, moving ? knot_t.data() : nullptr, moving ? poses.data() : nullptr,
                                            (int)knot_t.size(), ref_pose ? ref : nullptr, filter, signal ? sg.data() : nullptr,
                                            nir ? nr.data() : nullptr, &m);
    if (status_ != NDT_OK) return 0;
    if (signal) signal->assign(sg.begin(), sg.begin() + (std::ptrdiff_t)m);
    if (nir) nir->assign(nr.begin(), nr.begin() + (std::ptrdiff_t)m);
    return m;
  }
  // D(t) of that model as a matrix (host only)
  template <class Poses>
  static bool trajectoryPose(const std::vector<double>& knot_t, const Poses& knot_poses, double t, Matrix4d& out,
                             const Matrix4d* ref_pose = nullptr) {
    if (knot_t.size() != knot_poses.size()) return false;
    const std::vector<double> poses = detail::pack_poses(knot_poses);
    double ref[16], o[16];
    if (ref_pose) detail::to_colmajor(*ref_pose, 4, 4, ref);
    if (ndt_trajectory_pose(knot_t.data(), poses.data(), (int)knot_t.size(), ref_pose ? ref : nullptr, t, o) != NDT_OK) return false;
    out = detail::from_colmajor<Matrix4d>(o, 4, 4);
    return true;
  }

  // ---- clouds that are already in HBM (SoA float arrays on this engine's device) ----
  // the target arrays are consumed by the build; the source arrays are viewed in place until the source
  // is replaced (setInputSource's shared_ptr contract) -- or copied with copy = true
  // (deferred = true: the build is only enqueued -- the arrays must stay unchanged until align() / wait() has returned --
  // and the align's first evaluation goes onto the stream behind it: ndt_set_target_device_deferred)
  void setInputTargetDevice(const float* dx, const float* dy, const float* dz, size_t n, bool deferred = false) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    status_ = deferred ? ndt_set_target_device_deferred(h_, dx, dy, dz, n) : ndt_set_target_device(h_, dx, dy, dz, n);
  }
  void setInputSourceDevice(const float* dx, const float* dy, const float* dz, size_t n, bool copy = false) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    status_ = copy ? ndt_set_source_device(h_, dx, dy, dz, n) : ndt_set_source_device_view(h_, dx, dy, dz, n);
    if (status_ == NDT_OK) n_src_ = 0;  // align()'s output cloud is not filled on this path
  }

  // engine-specific: the hand-off of host clouds.  By default setInputTarget / setInputSource return as soon as the
  // caller's cloud has been consumed; the transfer and the voxel-grid build finish behind them and align() waits
  // (ndt_set_handoff_mode in ndt_hip.h).  wait() blocks until they are complete and reports a failed build.
  void setHandoffMode(int mode /* NDT_HANDOFF_ASYNC | NDT_HANDOFF_SYNC */) {
    status_ = h_ ? ndt_set_handoff_mode(h_, mode) : NDT_ERR_NO_DEVICE;
  }
  int wait() { return status_ = h_ ? ndt_wait(h_) : NDT_ERR_NO_DEVICE; }

  // engine-specific: 48-byte voxel records (f64 mean, f32 inverse covariance) instead of 80-byte f64 ones
  // (ndt_set_record_format in ndt_hip.h: what it costs in accuracy and what it saves per evaluation)
  void setPackedVoxelRecords(bool on) {
    status_ = h_ ? ndt_set_record_format(h_, on ? NDT_RECORDS_PACKED48 : NDT_RECORDS_F64) : NDT_ERR_NO_DEVICE;
  }

  // ---- multi-grid target [RECALLED: tier4 ndt_omp multigrid_ndt_omp.h -- addTarget / removeTarget /
  // createVoxelKdtree with string ids; the reference names the class only in its build,
  // CMakeLists.txt:41-42, and no driver instantiates it] ----
  template <class CloudPtrT>
  void addTarget(const CloudPtrT& cloud, const std::string& target_id) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    if (!cloud || cloud->points.empty()) { status_ = NDT_ERR_INVALID_ARG; return; }
    auto it = target_ids_.find(target_id);
    const int64_t id = it != target_ids_.end() ? it->second : next_target_id_++;
    status_ = ndt_multigrid_add_target(h_, id, &cloud->points[0].x, cloud->points.size(), sizeof(cloud->points[0]));
    if (status_ == NDT_OK) target_ids_[target_id] = id;
    grid_ = TargetGrid();
  }
  template <class CloudPtrT>
  void setInputTarget(const CloudPtrT& cloud, const std::string& target_id) { addTarget(cloud, target_id); }
  void removeTarget(const std::string& target_id) {
    auto it = target_ids_.find(target_id);
    if (!h_ || it == target_ids_.end()) { status_ = h_ ? NDT_ERR_INVALID_ARG : NDT_ERR_NO_DEVICE; return; }
    status_ = ndt_multigrid_remove_target(h_, it->second);
    target_ids_.erase(it);
    grid_ = TargetGrid();
  }
  void createVoxelKdtree() {
    status_ = h_ ? ndt_multigrid_create_kdtree(h_) : NDT_ERR_NO_DEVICE;
    grid_ = TargetGrid();
  }
  std::vector<std::string> getCurrentMapIDs() const {
    std::vector<std::string> v;
    for (const auto& kv : target_ids_) v.push_back(kv.first);
    return v;
  }

  int lastStatus() const { return status_; }
  std::string lastError() const { return h_ ? ndt_last_error(h_) : "no engine (ndt_create failed: GPU required)"; }
  const ndt_result& rawResult() const { return res_; }
  ndt_handle* handle() { return h_; }
  // `output` of align(): the drivers never read it (ref: run/pipeline.cpp:552,561), so it is
  // only produced (on the device) when asked for
  void setFillOutputCloud(bool on) { fill_output_ = on; }

 protected:
  // the engine call behind align(): GeneralizedIterativeClosestPoint below substitutes its own
  virtual int alignEngine(const float* guess, ndt_result* out) { return ndt_align(h_, guess, out); }
  void setStatus(int s) { status_ = s; }

 private:
  void push() { if (h_) status_ = ndt_set_params(h_, &prm_); }
  template <class Cloud>
  void uploadTarget(const Cloud* c) {
    if (!h_) return;
    status_ = (c && !c->points.empty())
                  ? ndt_set_target(h_, &c->points[0].x, c->points.size(), sizeof(c->points[0]))
                  : ndt_set_target(h_, nullptr, 0, 12);
  }
  template <class Cloud>
  void uploadSource(const Cloud* c) {
    if (!h_) return;
    n_src_ = c ? c->points.size() : 0;
    status_ = n_src_ ? ndt_set_source(h_, &c->points[0].x, n_src_, sizeof(c->points[0]))
                     : ndt_set_source(h_, nullptr, 0, 12);
  }
  template <class Cloud>
  bool scoreCloud(const Cloud& cloud, const Matrix4f& T, ndt_score* s) {
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return false; }
    uploadSource(&cloud);
    if (status_ != NDT_OK) return false;
    float a[16];
    detail::to_colmajor(T, 4, 4, a);
    status_ = ndt_score_transform(h_, a, s);
    return status_ == NDT_OK;
  }
  void run(const float* guess) {
    aligned_ = true;
    std::memset(&res_, 0, sizeof(res_));
    std::memcpy(res_.final_transformation, guess, sizeof(float) * 16);
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return; }
    status_ = alignEngine(guess, &res_);
    if (status_ != NDT_OK) {  // the reference returns the prior, not converged
      std::memcpy(res_.final_transformation, guess, sizeof(float) * 16);
      res_.converged = 0;
    }
  }
  void fillOutput(PointCloudSource& output) {
    if (!fill_output_ || !h_ || n_src_ == 0) return;
    std::vector<float> xyz(3 * n_src_);
    if (ndt_transform_source(h_, res_.final_transformation, xyz.data(), n_src_) != NDT_OK) return;
    output.points.resize(n_src_);
    for (size_t i = 0; i < n_src_; ++i) {
      output.points[i].x = xyz[3 * i];
      output.points[i].y = xyz[3 * i + 1];
      output.points[i].z = xyz[3 * i + 2];
    }
  }

  // both match calls: the bank's size, then every entry's result (h_ is set)
  ScanContextMatches scan_context_matches_(bool from_host, const float* desc, int64_t id) {
    ScanContextMatches out;
    const int64_t n = ndt_scan_context_bank_count(h_);
    if (n < 0) { status_ = (int)n; return out; }
    const size_t m = (size_t)n;
    out.ids.resize(m); out.distance.resize(m); out.shift.resize(m); out.columns.resize(m);
    const int64_t got = from_host ? ndt_scan_context_match(h_, desc, out.ids.data(), out.distance.data(), out.shift.data(),
                                                           out.columns.data(), m)
                                  : ndt_scan_context_match_keyframe(h_, id, out.ids.data(), out.distance.data(),
                                                                    out.shift.data(), out.columns.data(), m);
    status_ = got < 0 ? (int)got : NDT_OK;
    if (got != n) out = ScanContextMatches();
    return out;
  }

  ndt_params prm_{};
  ndt_handle* h_ = nullptr;
  ndt_result res_{};
  bool aligned_ = false;   // res_ holds an align's outcome (getFitnessScore's transform; identity before)
  int status_ = NDT_OK;
  size_t n_src_ = 0;
  bool fill_output_ = false;
  TargetGrid grid_;
  std::map<std::string, int64_t> target_ids_;  // multi-grid: tier4's string ids -> the C-ABI's integers
  int64_t next_target_id_ = 1;
};

// pclomp::GeneralizedIterativeClosestPoint (ref: include/registercallback.hpp:11-12, config/register_config.json:
// gicp_corr_dist_threshold, gicp_transform_epsilon) on the engine's GICP (ndt_gicp_*, ndt_align_gicp): PCL's setter names,
// the clouds, align(), getFinalTransformation(), hasConverged() and getFitnessScore() of the class above -- whose NDT
// setters stay available: the target's voxel grid is still built, and ndt_align on the same clouds is the cross-check.
// With PCL visible it is a pcl::Registration like the NDT class, so it can be stored in RegisterCallback::registration.
template <typename PointSource, typename PointTarget>
class GeneralizedIterativeClosestPoint : public NormalDistributionsTransform<PointSource, PointTarget> {
  using Ndt = NormalDistributionsTransform<PointSource, PointTarget>;

 public:
#if NDT_HIP_WITH_PCL
  using Ptr = typename std::pointer_traits<typename Ndt::Base::Ptr>::template rebind<GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
  using ConstPtr = typename std::pointer_traits<typename Ndt::Base::Ptr>::template rebind<const GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
#else
  using Ptr = std::shared_ptr<GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
  using ConstPtr = std::shared_ptr<const GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
#endif

  GeneralizedIterativeClosestPoint() {
    ndt_gicp_default_params(&gp_);
#if NDT_HIP_WITH_PCL
    this->reg_name_ = "ndt_hip::GeneralizedIterativeClosestPoint";
    this->max_iterations_ = gp_.max_iterations;
    this->transformation_epsilon_ = gp_.transformation_epsilon;
#endif
  }

  void setMaxCorrespondenceDistance(double d) { gp_.max_correspondence_distance = d; pushGicp(); }
  double getMaxCorrespondenceDistance() const { return gp_.max_correspondence_distance; }
  void setTransformationEpsilon(double e) {
#if NDT_HIP_WITH_PCL
    this->transformation_epsilon_ = e;
#endif
    gp_.transformation_epsilon = e;
    pushGicp();
  }
  void setCorrespondenceRandomness(int k) { gp_.k_neighbours = k; pushGicp(); }
  int getCorrespondenceRandomness() const { return gp_.k_neighbours; }
  void setMaximumIterations(int n) {   // the outer loop
#if NDT_HIP_WITH_PCL
    this->max_iterations_ = n;
#endif
    gp_.max_iterations = n;
    pushGicp();
  }
  void setMaximumOptimizerIterations(int n) { gp_.max_inner_iterations = n; pushGicp(); }
  int getMaximumOptimizerIterations() const { return gp_.max_inner_iterations; }
  // every GICP parameter at once (max_neighbour_distance, covariance_epsilon, ...)
  const ndt_gicp_params& gicpParams() const { return gp_; }
  void setGicpParams(const ndt_gicp_params& p) { gp_ = p; pushGicp(); }
  // outer / inner iterations, evaluations, pairs and points without a covariance of the last align()
  const ndt_gicp_info& gicpInfo() const { return info_; }

 protected:
  int alignEngine(const float* guess, ndt_result* out) override { return ndt_align_gicp(this->handle(), guess, out, &info_); }

 private:
  void pushGicp() { this->setStatus(this->handle() ? ndt_gicp_set_params(this->handle(), &gp_) : NDT_ERR_NO_DEVICE); }
  ndt_gicp_params gp_{};
  ndt_gicp_info info_{};
};

// Voxelised GICP (ndt_vgicp_*, ndt_align_vgicp): the GICP class above whose align() registers the source to one aggregate
// per target leaf -- no nearest-point pairing, ONE Newton loop.  That loop is the NDT loop and reads the handle's
// ndt_params, so setTransformationEpsilon and setMaximumIterations are the NDT class's again here (the GICP class's set
// its two-level loop, which this method does not have), beside setStepSize, setResolution and the rest; of the GICP
// parameters only those that decide the covariances matter (setCorrespondenceRandomness, setGicpParams).  The voxels are
// the target's NDT leaves: setResolution and setMinPointPerVoxel decide them.  The reference names no such class: there is
// no compat header.
template <typename PointSource, typename PointTarget>
class VoxelizedGeneralizedIterativeClosestPoint : public GeneralizedIterativeClosestPoint<PointSource, PointTarget> {
  using Ndt = NormalDistributionsTransform<PointSource, PointTarget>;

 public:
#if NDT_HIP_WITH_PCL
  using Ptr = typename std::pointer_traits<typename Ndt::Base::Ptr>::template rebind<VoxelizedGeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
  using ConstPtr = typename std::pointer_traits<typename Ndt::Base::Ptr>::template rebind<const VoxelizedGeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
#else
  using Ptr = std::shared_ptr<VoxelizedGeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
  using ConstPtr = std::shared_ptr<const VoxelizedGeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
#endif

  VoxelizedGeneralizedIterativeClosestPoint() {
#if NDT_HIP_WITH_PCL
    this->reg_name_ = "ndt_hip::VoxelizedGeneralizedIterativeClosestPoint";
    this->max_iterations_ = this->params().max_iterations;
    this->transformation_epsilon_ = this->params().trans_epsilon;
#endif
  }

  void setTransformationEpsilon(double e) { Ndt::setTransformationEpsilon(e); }
  void setMaximumIterations(int n) { Ndt::setMaximumIterations(n); }
  // the table's counters, the points without a covariance and the pairs of the last evaluation of the last align()
  const ndt_vgicp_info& vgicpInfo() const { return vinfo_; }

 protected:
  int alignEngine(const float* guess, ndt_result* out) override { return ndt_align_vgicp(this->handle(), guess, out, &vinfo_); }

 private:
  ndt_vgicp_info vinfo_{};
};

// tier4's class name for the multi-grid face [RECALLED]; here the same engine object carries both faces
template <typename PointSource, typename PointTarget>
using MultiGridNormalDistributionsTransform = NormalDistributionsTransform<PointSource, PointTarget>;

// ---------------------------------------------------------------------------------------------
// svn_ndt::SvnNormalDistributionsTransform-shaped adapter (ref: extern/svn_ndt/include/svn_ndt.h:
// 100-182; driver run/pipeline_lo_svn.cpp:299-320,387-388).  Stage 1 of every SVN iteration is
// one batched kernel launch.
struct SvnNdtResult {  // svn_ndt::SvnNdtResult (svn_ndt.h:40-51)
#if NDT_HIP_WITH_GTSAM
  gtsam::Pose3 final_pose;
#else
  Matrix4d final_pose{};
#endif
  Matrix6d final_covariance{};  // GTSAM tangent order [rot, trans]
  bool converged = false;
  int iterations = 0;
};

template <typename PointSource, typename PointTarget>
class SvnNormalDistributionsTransform {
 public:
  using PointCloudSource = PointCloud<PointSource>;
  using PointCloudTarget = PointCloud<PointTarget>;

  SvnNormalDistributionsTransform() {
    ndt_default_params(&prm_);
    prm_.hessian_mode = NDT_HESSIAN_GAUSS_NEWTON;  // svn_ndt.h:314
    prm_.add_ridge = 1;                            // svn_ndt_impl.hpp:650-653
    status_ = ndt_create(&prm_, &h_);
    ndt_svn_default_params(&svn_);
    updateNdtConstants();
  }
  ~SvnNormalDistributionsTransform() { ndt_destroy(h_); }
  SvnNormalDistributionsTransform(const SvnNormalDistributionsTransform&) = delete;
  SvnNormalDistributionsTransform& operator=(const SvnNormalDistributionsTransform&) = delete;

  // clamps as the reference's setters (svn_ndt.h:118-160)
  void setResolution(float r) { prm_.resolution = r; push(); }
  float getResolution() const { return prm_.resolution; }
  void setMinPointPerVoxel(int n) { prm_.min_points_per_voxel = n; push(); }
  void setOutlierRatio(double o) { prm_.outlier_ratio = o; push(); }
  double getOutlierRatio() const { return prm_.outlier_ratio; }
  void setNeighborhoodSearchMethod(NeighborSearchMethod m) { prm_.search_method = (int)m; push(); }
  void setNeighborhoodSearchMethod(SvnNeighborSearchMethod m) {
    prm_.search_method = m == SvnNeighborSearchMethod::KDTREE ? NDT_KDTREE
                       : m == SvnNeighborSearchMethod::DIRECT1 ? NDT_DIRECT1 : NDT_DIRECT7;
    push();
  }
  void setUseGaussNewtonHessian(bool on) { prm_.hessian_mode = on ? NDT_HESSIAN_GAUSS_NEWTON : NDT_HESSIAN_FULL; push(); }
  void setNumThreads(int n) { prm_.num_threads = n > 0 ? n : 1; push(); }
  int getNumThreads() const { return prm_.num_threads; }
  void setParticleCount(int k) { svn_.particle_count = k > 0 ? k : 1; }
  int getParticleCount() const { return svn_.particle_count; }
  void setMaxIterations(int n) { svn_.max_iterations = n > 0 ? n : 1; }
  int getMaxIterations() const { return svn_.max_iterations; }
  void setKernelBandwidth(double h) { svn_.kernel_bandwidth = h > 1e-9 ? h : 1e-9; }
  double getKernelBandwidth() const { return svn_.kernel_bandwidth; }
  void setStepSize(double s) { svn_.step_size = s > 0 ? s : 1e-6; }
  double getStepSize() const { return svn_.step_size; }
  void setEarlyStopThreshold(double t) { svn_.stop_threshold = t >= 0 ? t : 1e-4; }
  double getEarlyStopThreshold() const { return svn_.stop_threshold; }
  void setParticleSeed(uint64_t seed) { seed_ = seed; }  // the reference seeds from the wall clock (:712)

  template <class CloudPtr>
  void setInputTarget(const CloudPtr& cloud) {
    if (!h_) return;
    status_ = (cloud && !cloud->points.empty())
                  ? ndt_set_target(h_, &cloud->points[0].x, cloud->points.size(), sizeof(cloud->points[0]))
                  : ndt_set_target(h_, nullptr, 0, 12);
  }

  // align(source_cloud, prior_mean) with the prior as 16 column-major doubles
  template <class Cloud>
  SvnNdtResult align(const Cloud& source, const double prior_pose_colmajor[16]) {
    ndt_svn_result out;
    std::memset(&out, 0, sizeof(out));
    std::memcpy(out.final_pose, prior_pose_colmajor, sizeof(double) * 16);
    for (int i = 0; i < 6; ++i) out.final_covariance[7 * i] = 1.0;  // failure convention, ref :682-702
    if (!h_) {
      status_ = NDT_ERR_NO_DEVICE;
    } else {
      status_ = source.points.empty() ? ndt_set_source(h_, nullptr, 0, 12)
                                      : ndt_set_source(h_, &source.points[0].x, source.points.size(), sizeof(source.points[0]));
      n_source_ = status_ == NDT_OK ? source.points.size() : 0;
      if (status_ == NDT_OK && svn_.particle_count > 0) {
        std::vector<double> particles(16 * (size_t)svn_.particle_count);
        ndt_svn_sample_particles(prior_pose_colmajor, svn_.particle_count, seed_++, particles.data());
        ndt_svn_result tmp;
        status_ = ndt_svn_align(h_, &svn_, prior_pose_colmajor, particles.data(), &tmp);
        if (status_ == NDT_OK) out = tmp;
      }
    }
    SvnNdtResult r;
    const Matrix4d P = detail::from_colmajor<Matrix4d>(out.final_pose, 4, 4);
#if NDT_HIP_WITH_GTSAM
    r.final_pose = gtsam::Pose3(P);
#else
    r.final_pose = P;
#endif
    r.final_covariance = detail::from_rowmajor<Matrix6d>(out.final_covariance, 6, 6);
    r.converged = out.converged != 0;
    r.iterations = out.iterations;
    return r;
  }
#if NDT_HIP_WITH_GTSAM
  // the reference's signature (svn_ndt.h:178-181; call site run/pipeline_lo_svn.cpp:388)
  template <class Cloud>
  SvnNdtResult align(const Cloud& source, const gtsam::Pose3& prior_mean) {
    double a[16];
    detail::to_colmajor(prior_mean.matrix(), 4, 4, a);
    return align(source, a);
  }
#endif

  // ---- the reference's public math hook (round 5; ref: extern/svn_ndt/include/svn_ndt.h:186-206, svn_ndt_impl.hpp:518-668) ----
  // computeParticleDerivatives: NDT score, gradient and (Gauss-Newton, the svn default) Hessian of the source at the pose
  // p = [x, y, z, roll, pitch, yaw].  The reference takes the ORIGINAL points from its member input_ (set by align) and
  // the moved ones from `trans_cloud`; here the source is what setInputSource() / the last align() handed over and the
  // engine moves it itself -- trans_cloud is only checked for its size.  One launch (ndt_eval_derivatives, K = 1).
  template <class CloudPtr>
  void setInputSource(const CloudPtr& cloud) {
    if (!h_) return;
    status_ = cloud && !cloud->points.empty()
                  ? ndt_set_source(h_, &cloud->points[0].x, cloud->points.size(), sizeof(cloud->points[0]))
                  : ndt_set_source(h_, nullptr, 0, 12);
    n_source_ = status_ == NDT_OK && cloud ? cloud->points.size() : 0;
  }
  template <class Vec6, class Mat6, class Cloud>
  double computeParticleDerivatives(Vec6& score_gradient, Mat6& hessian, const Cloud& trans_cloud, const Vec6& p,
                                    bool compute_hessian = true) {
    double pose[6], words[NDT_EVAL_WORDS], score = 0.0, g[6], H[36];
    for (int i = 0; i < 6; ++i) { pose[i] = p[i]; score_gradient[i] = 0.0; }
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) hessian(r, c) = 0.0;
    if (!h_) { status_ = NDT_ERR_NO_DEVICE; return 0.0; }
    if (trans_cloud.points.size() != n_source_) { status_ = NDT_ERR_INVALID_ARG; return 0.0; }
    status_ = ndt_eval_derivatives(h_, pose, nullptr, 1, compute_hessian ? 1 : 0, words);
    if (status_ != NDT_OK) return 0.0;
    ndt_unpack_eval(words, &score, g, H);
    for (int i = 0; i < 6; ++i) score_gradient[i] = g[i];
    if (compute_hessian)
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) hessian(r, c) = H[6 * r + c];
    return score;
  }

  // ---- the reference's other public math hooks (ref: svn_ndt.h:208-276, svn_ndt_impl.hpp:214-500) ----
  // One point, one point-voxel pair, one pair of particles at a time, on the HOST, in the reference's own precision
  // (f32 products, f64 accumulation): the reference opens them to its tests, and so does the adapter -- the engine's
  // evaluation (k_derivatives; computeParticleDerivatives above) does not go through them.  The angle tables and the
  // Gaussian constants are the engine's (ndt_angle_tables, ndt_gauss_constants: what every launch receives), so a sum
  // of updateDerivatives over a cloud's pairs checks the kernel against the reference-shaped arithmetic
  // (tests/cpp/test_grid_queries.cpp).  Matrix arguments: anything with (row, col); vectors: anything with [i].
  void updateNdtConstants() { ndt_gauss_constants((double)prm_.resolution, prm_.outlier_ratio, &gauss_d1_, &gauss_d2_); }
  double gaussD1() const { return gauss_d1_; }
  double gaussD2() const { return gauss_d2_; }
  template <class Vec6>
  void computeAngleDerivatives(const Vec6& p, bool compute_hessian = true) {
    double pose[6];
    for (int i = 0; i < 6; ++i) pose[i] = p[i];
    ndt_angle_tables(pose, j_ang_, h_ang_);
    if (!compute_hessian) std::fill(h_ang_, h_ang_ + 45, 0.0f);
  }
  // Fills the ANGULAR entries of the 4 x 6 point Jacobian (the caller has set the translation block to identity, as in
  // the reference) and the 24 x 6 stack of second derivatives: block i (rows 4 i .. 4 i + 3), column j = d2 x' / dp_i dp_j.
  template <class Vec3, class PointGradient, class PointHessian>
  void computePointDerivatives(const Vec3& x, PointGradient& point_gradient, PointHessian& point_hessian, bool compute_hessian = true) const {
    const float xf[3] = {(float)x[0], (float)x[1], (float)x[2]};
    auto along = [&](const float* row) { return row[0] * xf[0] + row[1] * xf[1] + row[2] * xf[2]; };
    static const int where_j[8][2] = {{1, 3}, {2, 3}, {0, 4}, {1, 4}, {2, 4}, {0, 5}, {1, 5}, {2, 5}};   // (component, parameter)
    for (int k = 0; k < 8; ++k) point_gradient(where_j[k][0], where_j[k][1]) = along(j_ang_ + 3 * k);
    if (!compute_hessian) return;
    for (int r = 0; r < 24; ++r)
      for (int c = 0; c < 6; ++c) point_hessian(r, c) = 0.0f;
    // (parameter i, parameter j >= i, component): the table's rows in order; the roll-roll block has no x component
    static const int where_h[15][3] = {{3, 3, 1}, {3, 3, 2}, {3, 4, 1}, {3, 4, 2}, {3, 5, 1}, {3, 5, 2}, {4, 4, 0}, {4, 4, 1},
                                       {4, 4, 2}, {4, 5, 0}, {4, 5, 1}, {4, 5, 2}, {5, 5, 0}, {5, 5, 1}, {5, 5, 2}};
    for (int k = 0; k < 15; ++k) {
      const int i = where_h[k][0], j = where_h[k][1], comp = where_h[k][2];
      const float v = along(h_ang_ + 3 * k);
      point_hessian(4 * i + comp, j) = v;
      if (i != j) point_hessian(4 * j + comp, i) = v;
    }
  }
  // One point-voxel pair: adds its share to score_gradient / hessian and returns its score (Magnusson eq. 6.9, 6.12, 6.13).
  template <class Vec6, class Mat6, class PointGradient, class PointHessian, class Vec3, class Mat3>
  double updateDerivatives(Vec6& score_gradient, Mat6& hessian, const PointGradient& point_gradient4, const PointHessian& point_hessian,
                           const Vec3& x_trans, const Mat3& c_inv, bool compute_hessian = true, bool use_gauss_newton_hessian = true) const {
    const double d[3] = {x_trans[0], x_trans[1], x_trans[2]};
    double cd[3];
    for (int r = 0; r < 3; ++r) cd[r] = c_inv(r, 0) * d[0] + c_inv(r, 1) * d[1] + c_inv(r, 2) * d[2];
    double q = d[0] * cd[0] + d[1] * cd[1] + d[2] * cd[2];
    if (!std::isfinite(q) || q < -1e-9) return 0.0;
    if (q < 0.0) q = 0.0;
    const double arg = gauss_d2_ * q * 0.5;
    if (arg > 50.0) return 0.0;
    const double e = std::exp(-arg), score_inc = -gauss_d1_ * e, factor = gauss_d1_ * gauss_d2_ * e;
    if (!std::isfinite(factor) || std::fabs(factor) < 1e-15) return score_inc;
    const float df[3] = {(float)d[0], (float)d[1], (float)d[2]};
    float cj[3][6], row[6];   // C^-1 J (f32), (x - mu)^T C^-1 J
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 6; ++c)
        cj[r][c] = (float)c_inv(r, 0) * point_gradient4(0, c) + (float)c_inv(r, 1) * point_gradient4(1, c) + (float)c_inv(r, 2) * point_gradient4(2, c);
    bool fin = true;
    for (int c = 0; c < 6; ++c) {
      row[c] = df[0] * cj[0][c] + df[1] * cj[1][c] + df[2] * cj[2][c];
      fin = fin && std::isfinite(factor * (double)row[c]);
    }
    if (fin)
      for (int c = 0; c < 6; ++c) score_gradient[c] += factor * (double)row[c];
    if (!compute_hessian) return score_inc;
    double add[6][6];
    float dc[3];   // (x - mu)^T C^-1 (f32)
    for (int c = 0; c < 3; ++c) dc[c] = df[0] * (float)c_inv(0, c) + df[1] * (float)c_inv(1, c) + df[2] * (float)c_inv(2, c);
    fin = true;
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) {
        const float jcj = point_gradient4(0, i) * cj[0][j] + point_gradient4(1, i) * cj[1][j] + point_gradient4(2, i) * cj[2][j];
        double t = (double)jcj;
        if (!use_gauss_newton_hessian) {
          const int a = i < j ? i : j, b = i < j ? j : i;   // (the stack is filled for both orders; the reference reads the upper one)
          const float third = dc[0] * point_hessian(4 * a + 0, b) + dc[1] * point_hessian(4 * a + 1, b) + dc[2] * point_hessian(4 * a + 2, b);
          t += -gauss_d2_ * ((double)row[i] * (double)row[j]) + (double)third;
        }
        add[i][j] = t * factor;
        fin = fin && std::isfinite(add[i][j]);
      }
    if (fin)
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) hessian(i, j) += add[i][j];
    return score_inc;
  }
  // k(l, k) = exp(-|Log(l^-1 k)|^2 / h) and its gradient with respect to l in l's tangent space ([rotation, translation],
  // gtsam's order), evaluated by the engine's own Stage-2 arithmetic (ndt_svn_rbf_kernel).  Pose3: anything with matrix();
  // h: setKernelBandwidth.  The gradient comes back as Vec6 (default: six doubles in a std::array).
  template <class Pose3>
  double rbf_kernel(const Pose3& pose_l, const Pose3& pose_k) const {
    double a[16], b[16], k = 0.0;
    pose_matrix(pose_l, a);
    pose_matrix(pose_k, b);
    ndt_svn_rbf_kernel(a, b, svn_.kernel_bandwidth, &k, nullptr);
    return k;
  }
  template <class Vec6 = std::array<double, 6>, class Pose3>
  Vec6 rbf_kernel_gradient(const Pose3& pose_l, const Pose3& pose_k) const {
    double a[16], b[16], k = 0.0, g[6];
    pose_matrix(pose_l, a);
    pose_matrix(pose_k, b);
    ndt_svn_rbf_kernel(a, b, svn_.kernel_bandwidth, &k, g);
    Vec6 out{};
    for (int i = 0; i < 6; ++i) out[i] = g[i];
    return out;
  }

  int lastStatus() const { return status_; }
  std::string lastError() const { return h_ ? ndt_last_error(h_) : "no engine (ndt_create failed: GPU required)"; }
  ndt_handle* handle() { return h_; }

 private:
  void push() { if (h_) status_ = ndt_set_params(h_, &prm_); updateNdtConstants(); }
  template <class Pose3>
  static void pose_matrix(const Pose3& p, double T[16]) {
    const auto M = p.matrix();
    for (int c = 0; c < 4; ++c)
      for (int r = 0; r < 4; ++r) T[4 * c + r] = M(r, c);
  }
  double gauss_d1_ = 0.0, gauss_d2_ = 0.0;
  float j_ang_[24] = {}, h_ang_[45] = {};
  size_t n_source_ = 0;
  ndt_params prm_{};
  ndt_svn_params svn_{};
  ndt_handle* h_ = nullptr;
  int status_ = NDT_OK;
  uint64_t seed_ = 1;
};

}  // namespace ndt_hip
