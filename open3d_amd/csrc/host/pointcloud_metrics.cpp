// Host drivers of PointCloud::ComputeMetrics (t/geometry/PointCloud.cpp:
// 1805-1836, t/geometry/kernel/Metrics.cpp) and of the per-point distances of
// ComputePointCloudDistance (geometry/PointCloud.cpp:133-157). Arguments are
// checked before anything is allocated or launched; the kernels are in
// pointcloud_metrics.hip, the index build in nns.hip.
#include <algorithm>
#include <vector>

#include "../pointcloud_metrics.h"
#include "o3d_mi355x_host.h"
#include "pointcloud_call.h"

using namespace o3dmi;

namespace {

// The number of values the metric list expands to, or -1 for a list that is
// refused (the message is recorded).
int64_t CountValues(const int32_t* metrics, int n_metrics, int n_radii) {
    if (n_metrics < 0 || n_radii < 0 || (n_metrics > 0 && !metrics)) {
        SetLastError("metrics: null list or negative count");
        return -1;
    }
    int64_t values = 0;
    for (int k = 0; k < n_metrics; ++k) {
        if (metrics[k] < O3DMI_METRIC_CHAMFER_DISTANCE ||
            metrics[k] > O3DMI_METRIC_FSCORE) {
            SetLastError("metrics: unknown metric code");
            return -1;
        }
        if (metrics[k] == O3DMI_METRIC_FSCORE && n_radii < 1) {
            SetLastError("metrics: FScore needs at least one radius");
            return -1;
        }
        values += metrics[k] == O3DMI_METRIC_FSCORE ? n_radii : 1;
    }
    return values;
}

// ComputeMetricsCommon (t/geometry/kernel/Metrics.cpp:16-66), statement for
// statement, on the sums instead of the distance tensors. Index 0 is the
// direction cloud 1 -> cloud 2 (upstream's distance12, n1 entries).
void ValuesFromSums(int64_t n1, int64_t n2, const double* sum,
                    const double* max, const int64_t* counts, int n_radii,
                    const int32_t* metrics, int n_metrics, float* values) {
    const float mean12 = (float)(sum[0] / (double)n1);
    const float mean21 = (float)(sum[1] / (double)n2);
    float metric_val;
    int64_t idx = 0;
    for (int k = 0; k < n_metrics; ++k) {
        switch (metrics[k]) {
            case O3DMI_METRIC_CHAMFER_DISTANCE:
                metric_val = mean21 + mean12;
                values[idx++] = metric_val;
                break;
            case O3DMI_METRIC_HAUSDORFF_DISTANCE:
                metric_val = std::max((float)max[0], (float)max[1]);
                values[idx++] = metric_val;
                break;
            default:  // O3DMI_METRIC_FSCORE
                for (int r = 0; r < n_radii; ++r) {
                    float precision = (float)counts[r];
                    float recall = (float)counts[n_radii + r];
                    precision *= 100. / (double)n1;
                    recall *= 100. / (double)n2;
                    float fscore = 0.0;
                    if (precision + recall > 0) {
                        fscore = 2 * precision * recall / (precision + recall);
                    }
                    values[idx++] = fscore;
                }
                break;
        }
    }
}

int CheckCloud(const void* points_dev, int64_t n) {
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(n > 0, "One or both input point clouds are empty!");
    O3DMI_REQUIRE(points_dev != nullptr, "null argument");
    O3DMI_REQUIRE(n < (1ll << 31) - 1, "n out of range (< 2^31 - 1 points)");
    return O3DMI_OK;
}

// What one direction of ComputeMetrics leaves on the host.
struct Direction {
    double sum = 0, max = 0;
    int64_t second_pass = 0;
    std::vector<int64_t> counts;
};

// Nearest-point distances of `queries` in `target` and their reduction.
int RunDirection(const void* target_dev, int64_t n, const void* queries_dev,
                 int64_t q, int dtype, const float* radii, int n_radii,
                 Direction* out, hipStream_t s) {
    PoolScratch pool(s);
    const int groups = std::max(
            1, (n_radii + kMetricsRadiusGroup - 1) / kMetricsRadiusGroup);
    void* d2 = nullptr;
    MetricsWords* words = nullptr;
    double* sums = nullptr;
    int st = pool.Alloc(&d2, ElemSize(dtype) * (size_t)q);
    if (!st) st = pool.Alloc(&words, sizeof(MetricsWords) * (size_t)groups);
    if (!st)
        st = pool.Alloc(&sums, sizeof(double) * MetricsSumScratchDoubles(q));
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(words, 0,
                                   sizeof(MetricsWords) * (size_t)groups, s));
    st = NearestSearchRun(target_dev, n, queries_dev, q, dtype, d2, nullptr,
                          &out->second_pass, s);
    if (st) return st;
    const double* total = nullptr;
    for (int g = 0; g < groups; ++g) {
        const int first = g * kMetricsRadiusGroup;
        const int count = std::min(kMetricsRadiusGroup, n_radii - first);
        st = MetricsReduceAsync(d2, q, dtype, nullptr, radii + first,
                                count > 0 ? count : 0, g == 0, words + g, sums,
                                &total, s);
        if (st) return st;
    }
    std::vector<MetricsWords> host((size_t)groups);
    O3DMI_HIP_CHECK(hipMemcpyAsync(host.data(), words,
                                   sizeof(MetricsWords) * (size_t)groups,
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipMemcpyAsync(&out->sum, total, sizeof(double),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    std::memcpy(&out->max, &host[0].max_bits, sizeof(double));
    out->counts.resize((size_t)n_radii);
    for (int r = 0; r < n_radii; ++r)
        out->counts[(size_t)r] = (int64_t)host[(size_t)(r / kMetricsRadiusGroup)]
                                         .counts[r % kMetricsRadiusGroup];
    return O3DMI_OK;
}

}  // namespace

extern "C" {

int o3dmi_metrics_from_sums(int64_t n1, int64_t n2, const double sum[2],
                            const double max[2], const int64_t* counts,
                            int n_radii, const int32_t* metrics, int n_metrics,
                            float* values_out, int64_t values_capacity) {
    O3DMI_REQUIRE(n1 > 0 && n2 > 0,
                  "One or both input point clouds are empty!");
    O3DMI_REQUIRE(sum && max, "null argument");
    const int64_t values = CountValues(metrics, n_metrics, n_radii);
    if (values < 0) return O3DMI_ERR_INVALID_ARG;
    O3DMI_REQUIRE(n_radii == 0 || counts, "null argument");
    O3DMI_REQUIRE(values == 0 || values_out, "null argument");
    if (values_capacity < values) {
        SetLastError("metrics: values_capacity too small");
        return O3DMI_ERR_CAPACITY;
    }
    ValuesFromSums(n1, n2, sum, max, counts, n_radii, metrics, n_metrics,
                   values_out);
    return O3DMI_OK;
}

int o3dmi_pointcloud_nearest_distance(const void* target_dev, int64_t n,
                                      const void* queries_dev, int64_t q,
                                      int dtype, void* dist_out_dev,
                                      int32_t* idx_out_dev,
                                      o3dmi_stream_t stream) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    int st = CheckCloud(target_dev, n);
    if (st) return st;
    O3DMI_REQUIRE(q >= 0 && q < (1ll << 31) - 1, "q out of range");
    if (q == 0) return O3DMI_OK;
    O3DMI_REQUIRE(queries_dev && dist_out_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    MetricsWords* words = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = pool.Alloc(&words, sizeof(MetricsWords)))) return st;
    if ((st = RequireFinite(target_dev, n, dtype, w, s))) return st;
    if ((st = RequireFinite(queries_dev, q, dtype, w, s))) return st;
    // the squares land in the caller's array; the root is taken in place
    st = NearestSearchRun(target_dev, n, queries_dev, q, dtype, dist_out_dev,
                          idx_out_dev, nullptr, s);
    if (st) return st;
    st = MetricsReduceAsync(dist_out_dev, q, dtype, dist_out_dev, nullptr, 0,
                            false, words, nullptr, nullptr, s);
    if (st) return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_pointcloud_compute_metrics(
        const void* points1_dev, int64_t n1, const void* points2_dev,
        int64_t n2, int dtype, const int32_t* metrics, int n_metrics,
        const float* fscore_radius, int n_radii, float* values_out,
        int64_t values_capacity, o3dmi_pointcloud_metrics_raw_t* raw_out,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    int st = CheckCloud(points1_dev, n1);
    if (!st) st = CheckCloud(points2_dev, n2);
    if (st) return st;
    const int64_t values = CountValues(metrics, n_metrics, n_radii);
    if (values < 0) return O3DMI_ERR_INVALID_ARG;
    O3DMI_REQUIRE(n_radii == 0 || fscore_radius, "null argument");
    O3DMI_REQUIRE(values == 0 || values_out, "null argument");
    if (values_capacity < values) {
        SetLastError("metrics: values_capacity too small");
        return O3DMI_ERR_CAPACITY;
    }
    hipStream_t s = (hipStream_t)stream;
    Direction dir[2];
    {
        PoolScratch pool(s);
        Words* w = nullptr;
        if ((st = AllocWords(pool, &w))) return st;
        if ((st = RequireFinite(points1_dev, n1, dtype, w, s))) return st;
        if ((st = RequireFinite(points2_dev, n2, dtype, w, s))) return st;
    }
    st = RunDirection(points2_dev, n2, points1_dev, n1, dtype, fscore_radius,
                      n_radii, &dir[0], s);
    if (!st)
        st = RunDirection(points1_dev, n1, points2_dev, n2, dtype,
                          fscore_radius, n_radii, &dir[1], s);
    if (st) return st;
    const double sum[2] = {dir[0].sum, dir[1].sum};
    const double max[2] = {dir[0].max, dir[1].max};
    std::vector<int64_t> counts((size_t)(2 * n_radii));
    for (int r = 0; r < n_radii; ++r) {
        counts[(size_t)r] = dir[0].counts[(size_t)r];
        counts[(size_t)(n_radii + r)] = dir[1].counts[(size_t)r];
    }
    ValuesFromSums(n1, n2, sum, max, counts.data(), n_radii, metrics,
                   n_metrics, values_out);
    if (raw_out) {
        for (int d = 0; d < 2; ++d) {
            raw_out->sum[d] = sum[d];
            raw_out->max[d] = max[d];
            raw_out->second_pass_queries[d] = dir[d].second_pass;
        }
        if (raw_out->counts)
            std::copy(counts.begin(), counts.end(), raw_out->counts);
    }
    return O3DMI_OK;
}

}  // extern "C"
