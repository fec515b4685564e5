// Host drivers of PointCloud::SmoothLaplacian / SmoothTaubin / SmoothMLS /
// SmoothBilateral / ComputeBoundaryPoints and of the three normal calls
// (t/geometry/PointCloud.cpp:762-854, 986-1050, 1074-1203; the device
// drivers they call, t/geometry/kernel/PointCloudImpl.h:1410-1753).
// Arguments are checked before anything is allocated, launched or written;
// the kernels, the fused output policies of the searches among them, are in
// pointcloud_smooth.hip; the index and the plain searches in nns.hip.
#include <cmath>

#include "../pointcloud_smooth.h"
#include "../scan.h"
#include "o3d_mi355x.h"
#include "o3d_mi355x_host.h"
#include "pointcloud_call.h"

using namespace o3dmi;

namespace {

bool Overlap(const void* a, const void* b, size_t bytes) {
    if (!a || !b) return false;
    const char* x = (const char*)a;
    const char* y = (const char*)b;
    return x < y + bytes && y < x + bytes;
}

int CopyRows(void* dst, const void* src, int64_t n, int dtype, hipStream_t s) {
    O3DMI_HIP_CHECK(hipMemcpyAsync(dst, src, 3 * ElemSize(dtype) * (size_t)n,
                                   hipMemcpyDeviceToDevice, s));
    return O3DMI_OK;
}

// SmoothLaplacian (one factor) and SmoothTaubin (lambda, then mu): `passes`
// Laplacian passes whose factors alternate between f[0] and f[1].
int LaplacianPasses(const void* points_dev, int64_t n, int dtype,
                    int64_t iterations, const double* f, int per_iteration,
                    int max_nn, bool fixed, void* out_dev, hipStream_t s) {
    O3DMI_REQUIRE(n >= 0 && iterations >= 0, "n < 0 or iterations < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(points_dev && out_dev, "null argument");
    const size_t bytes = 3 * ElemSize(dtype) * (size_t)n;
    O3DMI_REQUIRE(!Overlap(points_dev, out_dev, bytes),
                  "out_points aliases points");
    if (iterations == 0 || max_nn <= 0) {
        int st = CopyRows(out_dev, points_dev, n, dtype, s);
        if (st) return st;
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        return O3DMI_OK;
    }
    if (max_nn > kMaxSmoothNeighbors - 1)
        return Unsupported("max_nn > 63 is not supported");
    O3DMI_REQUIRE(n < (1ll << 31) - 1, "too many points");
    O3DMI_REQUIRE(iterations < (1ll << 30), "too many iterations");
    const int k = (int)(n < (int64_t)max_nn + 1 ? n : (int64_t)max_nn + 1);
    const int64_t passes = iterations * per_iteration;
    PoolScratch pool(s);
    Words* w = nullptr;
    char* tmp = nullptr;
    int32_t* table = nullptr;
    int st = AllocWords(pool, &w);
    if (!st && passes > 1) st = pool.Alloc(&tmp, bytes);
    if (!st && fixed) st = pool.Alloc(&table, sizeof(int32_t) * (size_t)n * k);
    if (st) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    if (fixed) {
        st = o3dmi_nns_knn_search_counts(points_dev, n, points_dev, n, dtype, k,
                                         table, nullptr, nullptr,
                                         (o3dmi_stream_t)s);
        if (st) return st;
    }
    const void* cur = points_dev;
    for (int64_t t = 0; t < passes; ++t) {
        // the last pass lands in out_dev
        void* next = ((passes - 1 - t) & 1) ? (void*)tmp : out_dev;
        SmoothOp op{};
        op.kind = kSmoothLaplacian;
        op.points = cur;
        op.out_points = next;
        op.p0 = f[t % per_iteration];
        st = fixed ? TableSmoothOpAsync(op, table, nullptr, nullptr, nullptr, n,
                                        k, dtype, s)
                   : KnnSearchSmoothOp(cur, n, dtype, k, op, s);
        if (st) return st;
        cur = next;
    }
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

// Hybrid-search operators' shared argument checks (bilateral, boundary).
int CheckHybridArgs(const void* points_dev, const void* normals_dev, int64_t n,
                    int dtype, double radius, int max_nn) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(points_dev != nullptr, "points is null");
    O3DMI_REQUIRE(normals_dev != nullptr, "the cloud has no normals");
    O3DMI_REQUIRE(radius > 0, "radius must be positive");
    O3DMI_REQUIRE(max_nn >= 1, "max_nn must be positive");
    O3DMI_REQUIRE(n < (1ll << 31) - 1, "too many points");
    return O3DMI_OK;
}

}  // namespace

extern "C" {

int o3dmi_pointcloud_smooth_laplacian(const void* points_dev, int64_t n,
                                      int dtype, int64_t iterations,
                                      double lambda, int max_nn,
                                      int use_fixed_neighborhoods,
                                      void* out_points_dev,
                                      o3dmi_stream_t stream) {
    return LaplacianPasses(points_dev, n, dtype, iterations, &lambda, 1, max_nn,
                           use_fixed_neighborhoods != 0, out_points_dev,
                           (hipStream_t)stream);
}

int o3dmi_pointcloud_smooth_taubin(const void* points_dev, int64_t n, int dtype,
                                   int64_t iterations, double lambda, double mu,
                                   int max_nn, int use_fixed_neighborhoods,
                                   void* out_points_dev,
                                   o3dmi_stream_t stream) {
    const double f[2] = {lambda, mu};
    return LaplacianPasses(points_dev, n, dtype, iterations, f, 2, max_nn,
                           use_fixed_neighborhoods != 0, out_points_dev,
                           (hipStream_t)stream);
}

int o3dmi_pointcloud_smooth_mls(const void* points_dev, const void* normals_dev,
                                int64_t n, int dtype, double radius, int max_nn,
                                void* out_points_dev, void* out_normals_dev,
                                o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(points_dev && out_points_dev, "null argument");
    O3DMI_REQUIRE(!out_normals_dev || normals_dev,
                  "out_normals without normals");
    const size_t bytes = 3 * ElemSize(dtype) * (size_t)n;
    O3DMI_REQUIRE(!Overlap(out_points_dev, points_dev, bytes) &&
                          !Overlap(out_points_dev, normals_dev, bytes) &&
                          !Overlap(out_normals_dev, points_dev, bytes) &&
                          !Overlap(out_normals_dev, normals_dev, bytes) &&
                          !Overlap(out_normals_dev, out_points_dev, bytes),
                  "an output aliases an input");
    const bool hybrid = radius > 0.0 && max_nn > 0;
    const bool knn = !hybrid && max_nn > 0;
    if ((hybrid || knn) && max_nn > kMaxSmoothNeighbors)
        return Unsupported("max_nn > 64 is not supported");
    O3DMI_REQUIRE(n < (1ll << 31) - 1, "too many points");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    int st = AllocWords(pool, &w);
    if (st) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    // the index and the lists come first: the outputs are written only once
    // nothing but a launch can fail any more
    NnsGuard index;
    if (radius > 0.0 &&
        (st = o3dmi_nns_create(points_dev, n, dtype, radius, stream,
                               &index.nns)))
        return st;
    int64_t* splits = nullptr;
    int32_t* indices = nullptr;
    char* dist2 = nullptr;
    if (radius > 0.0 && !hybrid) {
        // FixedRadiusSearch: CSR rows (count pass, prefix sum, write pass)
        int32_t* counts = nullptr;
        char* scan_tmp = nullptr;
        st = pool.Alloc(&counts, sizeof(int32_t) * (size_t)n);
        if (!st) st = pool.Alloc(&splits, sizeof(int64_t) * (size_t)(n + 1));
        if (!st) st = pool.Alloc(&scan_tmp, ScanScratchBytes(n) + 256);
        if (st) return st;
        if ((st = o3dmi_nns_radius_count(index.nns, points_dev, n, counts,
                                         stream)))
            return st;
        O3DMI_HIP_CHECK(hipMemsetAsync(splits, 0, sizeof(int64_t), s));
        if ((st = PrefixSumAsync(counts, n, true, splits + 1, nullptr, scan_tmp,
                                 s)))
            return st;
        int64_t total = 0;
        O3DMI_HIP_CHECK(hipMemcpyAsync(&total, splits + n, sizeof(int64_t),
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        const size_t rows = (size_t)(total > 0 ? total : 1);
        st = pool.Alloc(&indices, sizeof(int32_t) * rows);
        if (!st) st = pool.Alloc(&dist2, ElemSize(dtype) * rows);
        if (st) return st;
        if ((st = o3dmi_nns_radius_search(index.nns, points_dev, n, splits,
                                          indices, dist2, stream)))
            return st;
    }
    if ((st = CopyRows(out_points_dev, points_dev, n, dtype, s))) return st;
    if (out_normals_dev &&
        (st = CopyRows(out_normals_dev, normals_dev, n, dtype, s)))
        return st;
    SmoothOp op{};
    op.kind = kSmoothMls;
    op.points = points_dev;
    op.out_points = out_points_dev;
    op.out_normals = out_normals_dev;
    op.p0 = radius;
    if (hybrid) {
        st = HybridSearchSmoothOp(index.nns, points_dev, n, max_nn, op, s);
    } else if (knn) {
        // BuildKnnNeighborhoods(points, max_nn - 1): k = min(n, max_nn), the
        // distances are zeros, so every weight is exp(-0)
        op.p0 = 0.0;
        st = KnnSearchSmoothOp(points_dev, n, dtype, max_nn, op, s);
    } else if (radius > 0.0) {
        st = TableSmoothOpAsync(op, indices, dist2, nullptr, splits, n, 0,
                                dtype, s);
    }
    if (st) return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    index.completed = true;
    return O3DMI_OK;
}

int o3dmi_pointcloud_smooth_bilateral(const void* points_dev,
                                      const void* normals_dev, int64_t n,
                                      int dtype, double radius, int max_nn,
                                      double sigma_s, double sigma_r,
                                      void* out_points_dev,
                                      o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(sigma_s > 0 && sigma_r > 0,
                  "Sigma values must be positive.");
    int st = CheckHybridArgs(points_dev, normals_dev, n, dtype, radius, max_nn);
    if (st) return st;
    O3DMI_REQUIRE(out_points_dev != nullptr, "null argument");
    const size_t bytes = 3 * ElemSize(dtype) * (size_t)n;
    O3DMI_REQUIRE(!Overlap(out_points_dev, points_dev, bytes) &&
                          !Overlap(out_points_dev, normals_dev, bytes),
                  "out_points aliases an input");
    if (max_nn > kMaxSmoothNeighbors)
        return Unsupported("max_nn > 64 is not supported");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    NnsGuard index;
    st = o3dmi_nns_create(points_dev, n, dtype, radius, stream, &index.nns);
    if (st) return st;
    if ((st = CopyRows(out_points_dev, points_dev, n, dtype, s))) return st;
    SmoothOp op{};
    op.kind = kSmoothBilateral;
    op.points = points_dev;
    op.normals = normals_dev;
    op.out_points = out_points_dev;
    op.p0 = sigma_s;
    op.p1 = sigma_r;
    st = HybridSearchSmoothOp(index.nns, points_dev, n, max_nn, op, s);
    if (st) return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    index.completed = true;
    return O3DMI_OK;
}

int o3dmi_pointcloud_compute_boundary_points(const void* points_dev,
                                             const void* normals_dev,
                                             int64_t n, int dtype,
                                             double radius, int max_nn,
                                             double angle_threshold,
                                             uint8_t* mask_out_dev,
                                             int64_t* m_out,
                                             o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    if (n == 0) {
        *m_out = 0;
        return O3DMI_OK;
    }
    int st = CheckHybridArgs(points_dev, normals_dev, n, dtype, radius, max_nn);
    if (st) return st;
    O3DMI_REQUIRE(mask_out_dev != nullptr, "null argument");
    const size_t bytes = 3 * ElemSize(dtype) * (size_t)n;
    O3DMI_REQUIRE(!Overlap(mask_out_dev, points_dev, bytes) &&
                          !Overlap(mask_out_dev, normals_dev, bytes),
                  "mask_out aliases an input");
    if (max_nn > kMaxSmoothNeighbors)
        return Unsupported("max_nn > 64 is not supported");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    NnsGuard index;
    st = o3dmi_nns_create(points_dev, n, dtype, radius, stream, &index.nns);
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(mask_out_dev, 0, (size_t)n, s));
    SmoothOp op{};
    op.kind = kSmoothBoundary;
    op.points = points_dev;
    op.normals = normals_dev;
    op.mask = mask_out_dev;
    op.p0 = angle_threshold;
    st = HybridSearchSmoothOp(index.nns, points_dev, n, max_nn, op, s);
    if (!st) st = CountMaskAsync(mask_out_dev, n, &w->count, s);
    if (!st) st = DownloadCount(w, m_out, s);
    index.completed = st == O3DMI_OK;  // the stream has drained
    return st;
}

int o3dmi_pointcloud_boundary_from_neighbors(
        const void* points_dev, const void* normals_dev,
        const int32_t* indices_dev, const int32_t* counts_dev, int64_t n,
        int nn_size, int dtype, double angle_threshold, uint8_t* mask_out_dev,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(nn_size >= 1, "nn_size must be positive");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(points_dev && normals_dev && indices_dev && counts_dev &&
                          mask_out_dev,
                  "null argument");
    if (nn_size > kMaxSmoothNeighbors)
        return Unsupported("nn_size > 64 is not supported");
    hipStream_t s = (hipStream_t)stream;
    O3DMI_HIP_CHECK(hipMemsetAsync(mask_out_dev, 0, (size_t)n, s));
    SmoothOp op{};
    op.kind = kSmoothBoundary;
    op.points = points_dev;
    op.normals = normals_dev;
    op.mask = mask_out_dev;
    op.p0 = angle_threshold;
    return TableSmoothOpAsync(op, indices_dev, nullptr, counts_dev, nullptr, n,
                              nn_size, dtype, s);
}

int o3dmi_pointcloud_normalize_normals(void* normals_dev, int64_t n, int dtype,
                                       o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "normals must be Float32 or Float64");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(normals_dev != nullptr, "the cloud has no normals");
    return NormalizeNormalsAsync(normals_dev, n, dtype, (hipStream_t)stream);
}

int o3dmi_pointcloud_orient_normals_to_align_with_direction(
        void* normals_dev, int64_t n, int dtype, const double* direction3,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "normals must be Float32 or Float64");
    O3DMI_REQUIRE(direction3 != nullptr, "direction is null");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(normals_dev != nullptr,
                  "No normals in the PointCloud. Call EstimateNormals() first.");
    return OrientNormalsToDirectionAsync(normals_dev, n, dtype, direction3,
                                         (hipStream_t)stream);
}

int o3dmi_pointcloud_orient_normals_towards_camera_location(
        const void* points_dev, void* normals_dev, int64_t n, int dtype,
        const double* camera3, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "normals must be Float32 or Float64");
    O3DMI_REQUIRE(camera3 != nullptr, "camera location is null");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(normals_dev != nullptr,
                  "No normals in the PointCloud. Call EstimateNormals() first.");
    O3DMI_REQUIRE(points_dev != nullptr, "points is null");
    return OrientNormalsToCameraAsync(points_dev, normals_dev, n, dtype,
                                      camera3, (hipStream_t)stream);
}

// Internal (tools/bench_pointcloud_smooth.py: the chain a seam-by-seam port
// would run): one operator over a neighbour table some search has written --
// rows of `width` entries with counts_dev {n} (NULL: every row is full).
// kind, p0, p1: SmoothOpKind and its parameters. out_points / out_normals
// must hold copies of the inputs for MLS and bilateral, mask zeros for the
// boundary test. Nothing is checked beyond the pointers; queued on the stream.
int o3dmi_internal_pointcloud_smooth_from_neighbors(
        int kind, const void* points_dev, const void* normals_dev,
        const int32_t* indices_dev, const void* dist2_dev,
        const int32_t* counts_dev, int64_t n, int width, int dtype, double p0,
        double p1, void* out_points_dev, void* out_normals_dev,
        uint8_t* mask_dev, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(kind >= kSmoothLaplacian && kind <= kSmoothBoundary,
                  "unknown operator");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(n >= 0 && width >= 1, "bad sizes");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(points_dev && indices_dev &&
                          (kind == kSmoothBoundary ? (void*)mask_dev
                                                   : out_points_dev),
                  "null argument");
    O3DMI_REQUIRE(normals_dev ||
                          (kind != kSmoothBilateral && kind != kSmoothBoundary),
                  "the cloud has no normals");
    SmoothOp op{};
    op.kind = kind;
    op.points = points_dev;
    op.normals = normals_dev;
    op.out_points = out_points_dev;
    op.out_normals = out_normals_dev;
    op.mask = mask_dev;
    op.p0 = p0;
    op.p1 = p1;
    return TableSmoothOpAsync(op, indices_dev, dist2_dev, counts_dev, nullptr,
                              n, width, dtype, (hipStream_t)stream);
}

}  // extern "C"
