// Compatibility header: `#include <pclomp/gicp_omp.h>` resolving to the MI355X engine.
//
// The reference's registration boundary includes this header beside the NDT ones
// (ref: include/registercallback.hpp:11-12) and its configuration carries gicp_corr_dist_threshold and
// gicp_transform_epsilon (ref: config/register_config.json).  With `include/compat` on the include path in front of
// the un-vendored ndt_omp headers, `pclomp::GeneralizedIterativeClosestPoint` is the HIP engine's GICP
// (ndt_hip::GeneralizedIterativeClosestPoint: PCL's setter names, a pcl::Registration when PCL is visible).  Written from
// the include names and PCL's public method names; nothing here comes from ndt_omp (its sources are absent from the
// reference tree).
#pragma once

#include "../../ndt_hip/ndt_hip.hpp"

namespace pclomp {

template <typename PointSource, typename PointTarget>
using GeneralizedIterativeClosestPoint = ndt_hip::GeneralizedIterativeClosestPoint<PointSource, PointTarget>;

}  // namespace pclomp
