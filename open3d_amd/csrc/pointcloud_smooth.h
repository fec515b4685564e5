// Private seam between the kernels of PointCloud::Smooth* / ComputeBoundary
// Points / the normal orientation calls (pointcloud_smooth.hip) and their C
// ABI in host/pointcloud_smooth.cpp. Every launcher is stream-ordered and waits for
// nothing unless it says so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct o3dmi_nns;

namespace o3dmi {

// One wave holds a point's neighbour list: widths the fused kernels accept.
constexpr int kMaxSmoothNeighbors = 64;

enum SmoothOpKind {
    kSmoothLaplacian = 0,  // p0 = factor
    kSmoothMls = 1,        // p0 = radius (<= 0: every weight is exp(-0))
    kSmoothBilateral = 2,  // p0 = sigma_s, p1 = sigma_r
    kSmoothBoundary = 3,   // p0 = angle threshold in degrees
};

// What a point's finished neighbour list is reduced to. Pointers are device
// memory in the point dtype; out_points / out_normals hold copies of the
// inputs for MLS and bilateral (the kernels write only the points they move),
// mask is zeroed (boundary).
struct SmoothOp {
    int kind;
    const void* points;
    const void* normals;
    void* out_points;
    void* out_normals;
    uint8_t* mask;
    double p0, p1;
};

// Fused forms: the search's output policy applies `op` to the list
// while it is in the wave's lanes; no {n, k} table exists.
// KNN over the cloud itself, k = min(n, knn) <= 64. Waits for the stream
// (the search's index is released on return).
int KnnSearchSmoothOp(const void* points_dev, int64_t n, int dtype, int knn,
                      const SmoothOp& op, hipStream_t s);
// Hybrid search of the cloud in its own index, max_knn <= 64.
int HybridSearchSmoothOp(const o3dmi_nns* nns, const void* points_dev,
                         int64_t n, int max_knn, const SmoothOp& op,
                         hipStream_t s);

// Table form: `op` over given lists -- rows of `width` entries with
// counts_dev {n} (NULL: every row is full), or CSR when row_splits_dev {n + 1}
// is given. dist2_dev may be NULL (all zero). Boundary needs width <= 64.
int TableSmoothOpAsync(const SmoothOp& op, const int32_t* indices_dev,
                       const void* dist2_dev, const int32_t* counts_dev,
                       const int64_t* row_splits_dev, int64_t n, int width,
                       int dtype, hipStream_t s);

// The three elementwise calls on normals {n,3}, in place
// (PointCloudImpl.h:229-350). vec3: the direction / camera location, host
// float64 {3}; it travels to the kernel by value in the point dtype.
int NormalizeNormalsAsync(void* normals_dev, int64_t n, int dtype,
                          hipStream_t s);
int OrientNormalsToDirectionAsync(void* normals_dev, int64_t n, int dtype,
                                  const double* vec3, hipStream_t s);
int OrientNormalsToCameraAsync(const void* points_dev, void* normals_dev,
                               int64_t n, int dtype, const double* vec3,
                               hipStream_t s);

}  // namespace o3dmi

// Entry point of host/pointcloud_smooth.cpp that is not in the public headers
// (described at its definition).
extern "C" int o3dmi_internal_pointcloud_smooth_from_neighbors(
        int kind, const void* points_dev, const void* normals_dev,
        const int32_t* indices_dev, const void* dist2_dev,
        const int32_t* counts_dev, int64_t n, int width, int dtype, double p0,
        double p1, void* out_points_dev, void* out_normals_dev,
        uint8_t* mask_dev, void* stream);
