// Host drivers of PointCloud::ClusterDBSCAN and PointCloud::SegmentPlane
// (legacy geometry/PointCloudCluster.cpp:21-97, geometry/PointCloud
// Segmentation.cpp:157-279; t/geometry/PointCloud.cpp:1634-1666 converts to
// the legacy cloud and calls them). Arguments are checked before anything is
// allocated or launched; the kernels are in pointcloud_segment.hip.
#include <cmath>
#include <vector>

#include "../pointcloud_segment.h"
#include "../scan.h"
#include "o3d_mi355x_host.h"
#include "pointcloud_call.h"

using namespace o3dmi;

namespace {

// GetPlaneFromPoints' closed form (PointCloudSegmentation.cpp:134-154).
void PlaneFromSums(const double sums[6], const double centroid[3],
                   double plane[4]) {
    double abc[3];
    PlaneNormalFromSums(sums, abc);
    const double norm =
            std::sqrt((abc[0] * abc[0] + abc[1] * abc[1]) + abc[2] * abc[2]);
    if (norm == 0 || !std::isfinite(norm)) {
        plane[0] = plane[1] = plane[2] = plane[3] = 0;
        return;
    }
    for (int k = 0; k < 3; ++k) plane[k] = abc[k] / norm;
    plane[3] = -((plane[0] * centroid[0] + plane[1] * centroid[1]) +
                 plane[2] * centroid[2]);
}

// The break bound after a new best (PointCloudSegmentation.cpp:238-248), with
// the cases upstream's cast leaves undefined mapped to num_iterations.
int64_t BreakIteration(double fitness, int ransac_n, double probability,
                       int64_t num_iterations) {
    if (!(fitness < 1.0)) return 0;
    const double den = std::log(1.0 - std::pow(fitness, (double)ransac_n));
    if (den == 0) return num_iterations;
    const double q = std::log(1.0 - probability) / den;
    if (!std::isfinite(q) || q < 0) return num_iterations;
    const double bound = q < (double)num_iterations ? q
                                                    : (double)num_iterations;
    return (int64_t)bound;
}

// Adds the rows of a {rows, 8} partial table in order.
void AddRows(const std::vector<double>& table, int64_t rows, int terms,
             double* out) {
    for (int k = 0; k < terms; ++k) out[k] = 0;
    for (int64_t r = 0; r < rows; ++r)
        for (int k = 0; k < terms; ++k) out[k] += table[8 * r + k];
}

struct Best {
    int64_t iteration = -1;
    double fitness = 0, rmse = 0;
};

}  // namespace

extern "C" {

int o3dmi_pointcloud_cluster_dbscan(const void* points_dev, int64_t n,
                                    int dtype, double eps, int64_t min_points,
                                    int32_t* labels_out_dev,
                                    int64_t* num_clusters_out,
                                    int64_t* num_noise_out,
                                    o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(eps > 0 && min_points >= 0,
                  "Illegal input parameters, eps must be positive and "
                  "min_points not negative");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(n == 0 || (points_dev && labels_out_dev), "null argument");
    if (n == 0) {
        if (num_clusters_out) *num_clusters_out = 0;
        if (num_noise_out) *num_noise_out = 0;
        return O3DMI_OK;
    }
    O3DMI_REQUIRE(n < (1ll << 27), "n out of range (< 2^27 points)");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    int32_t *counts = nullptr, *parent = nullptr, *root = nullptr,
            *is_root = nullptr;
    int64_t* cluster = nullptr;
    char* scan = nullptr;
    const size_t ints = sizeof(int32_t) * (size_t)n;
    int st = AllocWords(pool, &w);
    if (!st) st = pool.Alloc(&counts, ints);
    if (!st) st = pool.Alloc(&parent, ints);
    if (!st) st = pool.Alloc(&root, ints);
    if (!st) st = pool.Alloc(&is_root, ints);
    if (!st) st = pool.Alloc(&cluster, sizeof(int64_t) * (size_t)n);
    if (!st) st = pool.Alloc(&scan, ScanScratchBytes(n));
    if (st) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    NnsGuard index;
    st = o3dmi_nns_create(points_dev, n, dtype, eps, stream, &index.nns);
    if (st) return st;
    st = o3dmi_nns_radius_count(index.nns, points_dev, n, counts, stream);
    if (st) return st;
    // a count is in [1, n], n < 2^27
    const int need = min_points > n ? (int)(n + 1) : (int)min_points;
    if ((st = DbscanIdentityAsync(parent, n, s))) return st;
    st = DbscanUnionSweep(index.nns, points_dev, n, counts, need, parent, s);
    if (st) return st;
    st = DbscanFlattenAsync(parent, counts, need, n, root, is_root, s);
    if (st) return st;
    st = PrefixSumAsync(is_root, n, false, cluster, (int64_t*)&w->total, scan,
                        s);
    if (st) return st;
    st = DbscanLabelSweep(index.nns, points_dev, n, counts, need, root, cluster,
                          labels_out_dev, &w->count, s);
    if (st) return st;
    Words host;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&host, w, sizeof(Words),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    index.completed = true;  // the stream has drained
    if (num_clusters_out) *num_clusters_out = (int64_t)host.total;
    if (num_noise_out) *num_noise_out = (int64_t)host.count;
    return O3DMI_OK;
}

void o3dmi_plane_sample(uint64_t seed, int64_t iteration, int ransac_n,
                        int64_t n, int64_t* indices_out) {
    if (!indices_out || ransac_n < 1 || ransac_n > kPlaneMaxN ||
        n < ransac_n || iteration < 0)
        return;
    PlaneSample(seed, iteration, ransac_n, n, indices_out);
}

int o3dmi_plane_score(const void* points_dev, int64_t n, int dtype,
                      const double* planes_dev, int64_t b,
                      double distance_threshold, int64_t* counts_out_dev,
                      double* d2_sums_out_dev, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n >= 0 && b >= 0, "n < 0 or b < 0");
    O3DMI_REQUIRE(n < (1ll << 31) - 1, "too many points");
    O3DMI_REQUIRE(distance_threshold > 0, "distance_threshold must be > 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    if (b == 0) return O3DMI_OK;
    O3DMI_REQUIRE((n == 0 || points_dev) && planes_dev && counts_out_dev &&
                          d2_sums_out_dev,
                  "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int64_t cap = PlaneBatchCap(n);
    const int64_t rows = (b < cap ? b : cap) * (PlaneTiles(n) ? PlaneTiles(n)
                                                              : 1);
    PoolScratch pool(s);
    int32_t* part_counts = nullptr;
    double* part_sums = nullptr;
    int st = pool.Alloc(&part_counts, sizeof(int32_t) * (size_t)rows);
    if (!st) st = pool.Alloc(&part_sums, sizeof(double) * (size_t)rows);
    if (st) return st;
    for (int64_t at = 0; at < b; at += cap) {
        const int64_t count = b - at < cap ? b - at : cap;
        st = PlaneScoreAsync(points_dev, n, dtype, planes_dev + 4 * at, count,
                             distance_threshold, part_counts, part_sums,
                             counts_out_dev + at, d2_sums_out_dev + at, s);
        if (st) return st;
    }
    return O3DMI_OK;
}

int o3dmi_pointcloud_segment_plane(const void* points_dev, int64_t n,
                                   int dtype, double distance_threshold,
                                   int ransac_n, int64_t num_iterations,
                                   double probability, uint64_t seed,
                                   double plane_out[4],
                                   int64_t* inliers_out_dev, int64_t* m_out,
                                   o3dmi_segment_plane_info_t* info_out,
                                   o3dmi_stream_t stream) {
    O3DMI_REQUIRE(plane_out && m_out, "plane_out or m_out is null");
    O3DMI_REQUIRE(probability > 0 && probability <= 1,
                  "Probability must be > 0 and <= 1.0");
    O3DMI_REQUIRE(ransac_n >= 3,
                  "ransac_n should be set to higher than or equal to 3.");
    if (ransac_n > kPlaneMaxN)
        return Unsupported("ransac_n > 8 is not supported");
    O3DMI_REQUIRE(n >= ransac_n, "There must be at least 'ransac_n' points.");
    O3DMI_REQUIRE(num_iterations >= 1, "num_iterations must be >= 1");
    O3DMI_REQUIRE(distance_threshold > 0, "distance_threshold must be > 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(points_dev && inliers_out_dev, "null argument");
    O3DMI_REQUIRE(n < (1ll << 31) - 1, "too many points");
    hipStream_t s = (hipStream_t)stream;

    const int64_t cap = PlaneBatchCap(n);
    const int64_t max_batch = cap < num_iterations ? cap : num_iterations;
    const int64_t tiles = PlaneTiles(n);
    // one download per batch: {counts int64, sums float64, valid int32}
    const size_t result_bytes = (size_t)max_batch * 20;
    PoolScratch pool(s);
    Words* w = nullptr;
    double *planes = nullptr, *part_sums = nullptr, *refit = nullptr;
    int32_t *part_counts = nullptr, *flags = nullptr;
    int64_t* position = nullptr;
    char *results = nullptr, *scan = nullptr;
    int st = AllocWords(pool, &w);
    if (!st) st = pool.Alloc(&planes, sizeof(double) * 4 * (size_t)max_batch);
    if (!st) st = pool.Alloc(&results, result_bytes);
    if (!st)
        st = pool.Alloc(&part_counts,
                        sizeof(int32_t) * (size_t)(max_batch * tiles));
    if (!st)
        st = pool.Alloc(&part_sums,
                        sizeof(double) * (size_t)(max_batch * tiles));
    if (!st) st = pool.Alloc(&flags, sizeof(int32_t) * (size_t)n);
    if (!st) st = pool.Alloc(&position, sizeof(int64_t) * (size_t)n);
    if (!st) st = pool.Alloc(&scan, ScanScratchBytes(n));
    if (!st)
        st = pool.Alloc(&refit, sizeof(double) * 8 * (size_t)RefitBlocks(n));
    if (st) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;

    int64_t* counts_dev = (int64_t*)results;
    double* sums_dev = (double*)(results + 8 * (size_t)max_batch);
    int32_t* valid_dev = (int32_t*)(results + 16 * (size_t)max_batch);
    std::vector<char> host(result_bytes);
    const int64_t* counts = (const int64_t*)host.data();
    const double* sums = (const double*)(host.data() + 8 * (size_t)max_batch);
    const int32_t* valid =
            (const int32_t*)(host.data() + 16 * (size_t)max_batch);

    Best best;
    double best_plane[4] = {0, 0, 0, 0};
    int64_t counted = 0, break_iteration = num_iterations;
    int64_t first = 0;
    int64_t batch = 1024 < max_batch ? 1024 : max_batch;
    while (first < num_iterations && counted <= break_iteration) {
        const int64_t count = num_iterations - first < batch
                                      ? num_iterations - first
                                      : batch;
        st = PlaneHypothesesAsync(points_dev, n, dtype, seed, first, count,
                                  ransac_n, planes, valid_dev, s);
        if (st) return st;
        st = PlaneScoreAsync(points_dev, n, dtype, planes, count,
                             distance_threshold, part_counts, part_sums,
                             counts_dev, sums_dev, s);
        if (st) return st;
        O3DMI_HIP_CHECK(hipMemcpyAsync(host.data(), results, result_bytes,
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        // the reference loop, one thread, iteration order
        int64_t best_here = -1;
        for (int64_t k = 0; k < count; ++k) {
            if (counted > break_iteration) break;  // the rest is dropped
            if (!valid[k]) continue;               // zero plane: not counted
            double fitness = 0, rmse = 0;
            if (counts[k] > 0) {
                fitness = (double)counts[k] / (double)n;
                rmse = std::sqrt(sums[k] / (double)counts[k]);
            }
            if (fitness > best.fitness ||
                (fitness == best.fitness && rmse < best.rmse)) {
                best.iteration = first + k;
                best.fitness = fitness;
                best.rmse = rmse;
                best_here = k;
                break_iteration = BreakIteration(fitness, ransac_n,
                                                 probability, num_iterations);
            }
            ++counted;
        }
        if (best_here >= 0) {
            O3DMI_HIP_CHECK(hipMemcpyAsync(best_plane, planes + 4 * best_here,
                                           sizeof(best_plane),
                                           hipMemcpyDeviceToHost, s));
            O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        }
        first += count;
        batch = PlaneNextBatch(batch, max_batch, n);
    }

    int64_t m = 0;
    double plane[4] = {0, 0, 0, 0};
    if (best.iteration >= 0) {
        st = PlaneInlierFlagsAsync(points_dev, n, dtype, best_plane,
                                   distance_threshold, flags, s);
        if (st) return st;
        st = PrefixSumAsync(flags, n, false, position, (int64_t*)&w->total,
                            scan, s);
        if (st) return st;
        st = PlaneInlierIndicesAsync(flags, position, n, inliers_out_dev, s);
        if (st) return st;
        long long total = 0;
        O3DMI_HIP_CHECK(hipMemcpyAsync(&total, &w->total, sizeof(total),
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        m = (int64_t)total;
        // refit over the inliers: centroid, then the six centred sums
        const int64_t rows = RefitBlocks(m);
        std::vector<double> table(8 * (size_t)rows);
        double centroid[3] = {0, 0, 0}, sums6[6];
        for (int centred = 0; centred < 2 && m > 0; ++centred) {
            st = PlaneRefitSumsAsync(points_dev, dtype, inliers_out_dev, m,
                                     centred, centroid, refit, s);
            if (st) return st;
            O3DMI_HIP_CHECK(hipMemcpyAsync(table.data(), refit,
                                           sizeof(double) * table.size(),
                                           hipMemcpyDeviceToHost, s));
            O3DMI_HIP_CHECK(hipStreamSynchronize(s));
            if (centred) {
                AddRows(table, rows, 6, sums6);
            } else {
                AddRows(table, rows, 3, centroid);
                for (int k = 0; k < 3; ++k) centroid[k] /= (double)m;
            }
        }
        if (m > 0) PlaneFromSums(sums6, centroid, plane);
    }
    for (int k = 0; k < 4; ++k) plane_out[k] = plane[k];
    *m_out = m;
    if (info_out) {
        info_out->best_iteration = best.iteration;
        info_out->iterations_counted = counted;
        info_out->final_break_iteration = break_iteration;
        info_out->fitness = best.fitness;
        info_out->inlier_rmse = best.rmse;
    }
    return O3DMI_OK;
}

}  // extern "C"
