// Private seam between pointcloud_metrics.hip (the lane-group nearest-point
// search and the distance reduction) and host/pointcloud_metrics.cpp (the C ABI
// of PointCloud::ComputeMetrics / ComputePointCloudDistance). Every launcher is
// stream-ordered and waits for nothing.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "nns.h"

namespace o3dmi {

// Lanes that share a query in the first pass of the nearest-point search.
constexpr int kNearestGroup = 16;

// The first pass of NearestSearchRun (nns.h): a group of kNearestGroup lanes
// walks the finest level's growing cubes for a query and either writes its
// slot of d2_dev / idx_dev or appends the query to the retry list.
int NearestFirstPassAsync(const NearestFirstPass& fp, int dtype,
                          const void* queries_dev, int64_t q, void* d2_dev,
                          int32_t* idx_dev, hipStream_t s);

// ---- the reduction ----------------------------------------------------------
constexpr int kMetricsRun = 512;       // values added in index order per run
constexpr int kMetricsRadiusGroup = 8; // F-score radii counted per launch

// Doubles of scratch MetricsReduceAsync needs for q distances: the run sums of
// every level of the tree (the last level is the single total).
size_t MetricsSumScratchDoubles(int64_t q);

// The words a direction's reduction leaves on the device.
struct MetricsWords {
    unsigned long long max_bits;  // bits of the maximum as a double (d >= 0)
    unsigned long long counts[kMetricsRadiusGroup];
};

// d = SqrtOf(d2[i]) in the point dtype for i < q (written to dist_out_dev when
// given; it may be d2_dev itself). With n_radii <= kMetricsRadiusGroup radii:
// words->counts[r] += the number of d < radius[r] (strict; Float32 clouds
// compare in Float32, Float64 clouds with the radius widened). With
// `sum_and_max`: words->max_bits = max(max_bits, bits of (double)d), and
// *total_dev = the sum of (double)d in the fixed tree: consecutive runs of
// kMetricsRun values are added in index order, the run sums likewise, level by
// level until one value is left (*total_dev points into sums_dev). `words` is
// zeroed by the caller.
int MetricsReduceAsync(const void* d2_dev, int64_t q, int dtype,
                       void* dist_out_dev, const float* radii, int n_radii,
                       bool sum_and_max, MetricsWords* words_dev,
                       double* sums_dev, const double** total_dev,
                       hipStream_t s);

}  // namespace o3dmi
