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

// ---- exact nearest point of every query --------------------------------------
// d2_dev[i] = min over the n points of ((dx dx) + dy dy) + dz dz, dx = query -
// point, in the point dtype; idx_dev[i] (optional) = the lowest original index
// among the minima. A KNN search with knn = 1 (KnnSearchRun, nns_wave.h) whose
// first pass gives a group of kNearestGroup lanes to every query on the finest
// level. Waits for the stream (twice at least) and returns with the device
// drained; *second_pass_queries (optional) = the length of the retry list.
// Size limits and their errors are o3dmi_nns_knn_search's.
int NearestSearchRun(const void* points_dev, int64_t n, const void* queries_dev,
                     int64_t q, int dtype, void* d2_dev, int32_t* idx_dev,
                     int64_t* second_pass_queries, hipStream_t s);

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
