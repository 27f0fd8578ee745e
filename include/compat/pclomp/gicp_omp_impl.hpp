// Compatibility header (ref: include/registercallback.hpp:11-12): what pclomp's gicp_omp_impl.hpp would define that the
// reference's registration boundary can name lives in gicp_omp.h of this directory.
#pragma once
#include "gicp_omp.h"
