// Private seam between the kernels of PointCloud::ClusterDBSCAN /
// SegmentPlane (pointcloud_segment.hip) and their C ABI in
// host/pointcloud_segment.cpp. Every launcher is stream-ordered and waits for
// nothing.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ransac.h"

struct o3dmi_nns;

namespace o3dmi {

// ---- ClusterDBSCAN ---------------------------------------------------------
// Point i is a core point when counts[i] >= need (counts: o3dmi_nns_radius_
// count of the cloud in its own index, the point itself included).

// parent[i] = i.
int DbscanIdentityAsync(int32_t* parent_dev, int64_t n, hipStream_t s);

// Union sweep: one wave per core point i; every core candidate
// j < i within the index radius is united with i in parent[] (int32,
// identity beforehand). Afterwards the root of every tree is the lowest core
// index of its component.
int DbscanUnionSweep(const o3dmi_nns* nns, const void* points_dev, int64_t n,
                     const int32_t* counts_dev, int need, int32_t* parent_dev,
                     hipStream_t s);

// root[i] = root of core point i (-1 for the others); is_root[i] = 1 for a
// core point that is its own parent.
int DbscanFlattenAsync(const int32_t* parent_dev, const int32_t* counts_dev,
                       int need, int64_t n, int32_t* root_dev,
                       int32_t* is_root_dev, hipStream_t s);

// Label sweep. cluster_dev: exclusive prefix sum of is_root. Core
// points take cluster[root]; the others the smallest cluster[root[j]] over
// their core neighbours j, or -1. *noise_dev (zeroed by the caller) += the
// number of -1 labels, one atomic per wave.
int DbscanLabelSweep(const o3dmi_nns* nns, const void* points_dev, int64_t n,
                     const int32_t* counts_dev, int need,
                     const int32_t* root_dev, const int64_t* cluster_dev,
                     int32_t* labels_dev, unsigned long long* noise_dev,
                     hipStream_t s);

// ---- SegmentPlane ----------------------------------------------------------
constexpr int kPlaneMaxN = 8;     // sample size limit (O3DMI_RANSAC_MAX_N)
constexpr int kPlaneTile = 512;   // points per scoring tile
constexpr int kPlaneBlock = 256;  // hypotheses per scoring workgroup
constexpr int kRefitTile = 4096;  // inliers per refit workgroup

// Draws 0 .. ransac_n - 1 of iteration i over n points: draw k is uniform over
// the n - k points not drawn yet (RansacDraw's counter hash of (seed, i, k),
// mapped to [0, n - k) by the high half of the 128-bit product), then shifted
// past the earlier picks taken in ascending order. Exact sampling without
// replacement; ransac_n <= kPlaneMaxN <= n.
__host__ __device__ inline void PlaneSample(uint64_t seed, int64_t i,
                                            int ransac_n, int64_t n,
                                            int64_t* out) {
    int64_t sorted[kPlaneMaxN];
    for (int k = 0; k < ransac_n; ++k) {
        int64_t v = (int64_t)RansacDraw(seed, i, k, (uint64_t)(n - k));
        int at = 0;
        while (at < k && sorted[at] <= v) {
            ++v;
            ++at;
        }
        for (int m = k; m > at; --m) sorted[m] = sorted[m - 1];
        sorted[at] = v;
        out[k] = v;
    }
}

// GetPlaneFromPoints (PointCloudSegmentation.cpp:134-154) from the six centred
// sums {xx, xy, xz, yy, yz, zz}: the normal before it is normalised.
__host__ __device__ inline void PlaneNormalFromSums(const double* c,
                                                    double* abc) {
    const double xx = c[0], xy = c[1], xz = c[2], yy = c[3], yz = c[4],
                 zz = c[5];
    const double det_x = yy * zz - yz * yz;
    const double det_y = xx * zz - xz * xz;
    const double det_z = xx * yy - xy * xy;
    if (det_x > det_y && det_x > det_z) {
        abc[0] = det_x;
        abc[1] = xz * yz - xy * zz;
        abc[2] = xy * yz - xz * yy;
    } else if (det_y > det_z) {
        abc[0] = xz * yz - xy * zz;
        abc[1] = det_y;
        abc[2] = xy * xz - yz * xx;
    } else {
        abc[0] = xy * yz - xz * yy;
        abc[1] = xy * xz - yz * xx;
        abc[2] = det_z;
    }
}

inline int64_t PlaneTiles(int64_t n) {
    return (n + kPlaneTile - 1) / kPlaneTile;
}

// Hypotheses per scoring round: one partial per (hypothesis, tile), at most
// kRansacMaxPartials of them and at most kRansacMaxBatch hypotheses.
inline int64_t PlaneBatchCap(int64_t n) {
    const int64_t t = PlaneTiles(n) < 1 ? 1 : PlaneTiles(n);
    const int64_t c = kRansacMaxPartials / t;
    return c < 1 ? 1 : (c > kRansacMaxBatch ? kRansacMaxBatch : c);
}

// The driver's schedule: the batch doubles while a round stays below 2^30
// point-plane evaluations; never above the cap.
inline int64_t PlaneNextBatch(int64_t batch, int64_t cap, int64_t n) {
    if (batch * n < (1ll << 30)) batch *= 2;
    return batch > cap ? cap : batch;
}

// One thread per iteration first .. first + count - 1: sample, then
// ComputeTrianglePlane (ransac_n == 3) or GetPlaneFromPoints on the sample, in
// float64. planes_dev {count,4}; valid_dev[k] = 0 for a zero plane.
int PlaneHypothesesAsync(const void* points_dev, int64_t n, int dtype,
                         uint64_t seed, int64_t first, int64_t count,
                         int ransac_n, double* planes_dev, int32_t* valid_dev,
                         hipStream_t s);

// count and sum of d^2 of the points with d < threshold, for b <=
// PlaneBatchCap(n) planes. part_counts_dev int32 / part_sums_dev float64
// {PlaneTiles(n), b}: a tile's points are added in index order, the tiles in
// tile order.
int PlaneScoreAsync(const void* points_dev, int64_t n, int dtype,
                    const double* planes_dev, int64_t b, double threshold,
                    int32_t* part_counts_dev, double* part_sums_dev,
                    int64_t* counts_dev, double* d2_sums_dev, hipStream_t s);

// flags[i] = 1 when point i lies within threshold of `plane`.
int PlaneInlierFlagsAsync(const void* points_dev, int64_t n, int dtype,
                          const double plane[4], double threshold,
                          int32_t* flags_dev, hipStream_t s);
// indices[position[i]] = i for every flagged i (position: exclusive prefix
// sum of the flags): the inliers in ascending order.
int PlaneInlierIndicesAsync(const int32_t* flags_dev,
                            const int64_t* position_dev, int64_t n,
                            int64_t* indices_dev, hipStream_t s);

inline int64_t RefitBlocks(int64_t m) {
    return (m + kRefitTile - 1) / kRefitTile;
}
// Per-workgroup partial sums over the inliers, {RefitBlocks(m), 8} float64:
// centred == 0: {x, y, z}; else {xx, xy, xz, yy, yz, zz} of p - centroid.
// A thread adds its rows in index order, the workgroup's threads meet in a
// halving tree; the host adds the rows of the table in order.
int PlaneRefitSumsAsync(const void* points_dev, int dtype,
                        const int64_t* indices_dev, int64_t m, int centred,
                        const double centroid[3], double* partials_dev,
                        hipStream_t s);

}  // namespace o3dmi
