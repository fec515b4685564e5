// Host drivers of PointCloud::FarthestPointDownSample, UniformDownSample,
// RandomDownSample, Crop's two masks and GetMinBound / GetMaxBound
// (t/geometry/PointCloud.cpp:569-648). Arguments are checked before anything
// is allocated or launched; the kernels are in pointcloud_sample.hip.
#include <cmath>

#include "../pointcloud_sample.h"
#include "../ransac.h"
#include "o3d_mi355x_host.h"
#include "pointcloud_call.h"

using namespace o3dmi;

namespace {

// What both farthest-point calls refuse before anything is launched.
int CheckFarthestArgs(const void* points_dev, int64_t n, int dtype,
                      int64_t num_samples, int64_t start_index) {
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(num_samples >= 0 && num_samples <= n,
                  "Illegal number of samples, must be <= point size");
    O3DMI_REQUIRE(n == 0 || (start_index >= 0 && start_index < n),
                  "Illegal start index, must be < point size");
    O3DMI_REQUIRE(n == 0 || points_dev, "null argument");
    O3DMI_REQUIRE(n < (1ll << 27), "n out of range (< 2^27 points)");
    return O3DMI_OK;
}

// The order of a checked, finite cloud with n >= 1 and k >= 1, in the form
// asked for; scratch comes from the caller's pool.
int FarthestOrder(const void* points_dev, int64_t n, int dtype, int64_t k,
                  int64_t start, int form, int64_t* order_dev,
                  PoolScratch& pool, hipStream_t s) {
    const bool resident =
            form == 1 || (form == 0 && n <= FarthestResidentCapacity(dtype));
    if (resident)
        return FarthestOrderResidentAsync(points_dev, n, dtype, k, start,
                                          order_dev, s);
    char* scratch = nullptr;
    int st = pool.Alloc(&scratch, FarthestStreamScratchBytes(n, dtype));
    if (st) return st;
    return FarthestOrderStreamedAsync(points_dev, n, dtype, k, start,
                                      order_dev, scratch, s);
}

int CheckBox(const void* points_dev, int64_t n, int dtype,
             const uint8_t* mask_out_dev, const int64_t* m_out) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(n == 0 || (points_dev && mask_out_dev), "null argument");
    return O3DMI_OK;
}

}  // namespace

extern "C" {

int64_t o3dmi_pointcloud_farthest_point_capacity(int dtype) {
    return FarthestResidentCapacity(dtype);
}

int o3dmi_pointcloud_farthest_point_order(const void* points_dev, int64_t n,
                                          int dtype, int64_t num_samples,
                                          int64_t start_index, int form,
                                          int64_t* order_out_dev,
                                          o3dmi_stream_t stream) {
    int st = CheckFarthestArgs(points_dev, n, dtype, num_samples, start_index);
    if (st) return st;
    O3DMI_REQUIRE(form >= 0 && form <= 2, "form must be 0, 1 or 2");
    O3DMI_REQUIRE(num_samples == 0 || order_out_dev, "null argument");
    if (form == 1 && n > FarthestResidentCapacity(dtype))
        return Unsupported("farthest point: cloud above the resident capacity");
    if (num_samples == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    st = FarthestOrder(points_dev, n, dtype, num_samples, start_index, form,
                       order_out_dev, pool, s);
    if (st) return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_pointcloud_farthest_point_down_sample(
        const void* points_dev, int64_t n, int dtype, int64_t num_samples,
        int64_t start_index, uint8_t* mask_out_dev, int64_t* order_out_dev,
        int64_t* m_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    int st = CheckFarthestArgs(points_dev, n, dtype, num_samples, start_index);
    if (st) return st;
    O3DMI_REQUIRE(n == 0 || mask_out_dev, "null argument");
    if (n == 0) {
        *m_out = 0;
        return O3DMI_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    int64_t* order = order_out_dev;
    const bool whole = num_samples == n;  // upstream's Clone()
    const bool loop = num_samples > 0 && (!whole || order_out_dev);
    st = AllocWords(pool, &w);
    if (!st && loop && !order)
        st = pool.Alloc(&order, sizeof(int64_t) * (size_t)num_samples);
    if (st) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    if (loop) {
        st = FarthestOrder(points_dev, n, dtype, num_samples, start_index, 0,
                           order, pool, s);
        if (st) return st;
    }
    if (whole || num_samples == 0) {
        O3DMI_HIP_CHECK(hipMemsetAsync(mask_out_dev, whole ? 1 : 0, (size_t)n,
                                       s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        *m_out = num_samples;
        return O3DMI_OK;
    }
    // upstream: selection_mask[farthest_index] = true, sample after sample
    O3DMI_HIP_CHECK(hipMemsetAsync(mask_out_dev, 0, (size_t)n, s));
    if ((st = IndexToMaskAsync(order, num_samples, mask_out_dev, s))) return st;
    if ((st = CountMaskAsync(mask_out_dev, n, &w->count, s))) return st;
    return DownloadCount(w, m_out, s);
}

int o3dmi_pointcloud_uniform_down_sample(int64_t n, int64_t every_k_points,
                                         int n_attrs,
                                         const void* const* attrs_in,
                                         const int64_t* row_bytes,
                                         void* const* attrs_out,
                                         int64_t* m_out,
                                         o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(every_k_points >= 1,
                  "Illegal sample rate, every_k_points must be larger than 0.");
    SelectAttrs attrs;
    int st = CheckAttrs(n_attrs, attrs_in, row_bytes, attrs_out, n > 0,
                        &attrs);
    if (st) return st;
    // ceil(n / k) without n + k overflowing
    const int64_t m = n == 0 ? 0 : (n - 1) / every_k_points + 1;
    *m_out = m;
    if (m == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    if ((st = StridedRowsAsync(m, every_k_points, attrs, s))) return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int64_t o3dmi_sample_index(uint64_t seed, int64_t n, int64_t j) {
    if (j < 0 || j >= n || n >= (1ll << 62)) return -1;
    return SampleIndex(seed, n, j);
}

int o3dmi_pointcloud_random_sample_indices(int64_t n, double sampling_ratio,
                                           uint64_t seed,
                                           int64_t* indices_out_dev,
                                           int64_t* m_out,
                                           o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(sampling_ratio >= 0 && sampling_ratio <= 1,
                  "Illegal sampling_ratio, must be between 0 and 1.");
    O3DMI_REQUIRE(n < (1ll << 53), "too many points");  // ratio * n is exact
    const int64_t m = (int64_t)(sampling_ratio * (double)n);
    O3DMI_REQUIRE(m == 0 || indices_out_dev, "null argument");
    *m_out = m;
    if (m == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    int st = SampleIndicesAsync(seed, n, m, indices_out_dev, s);
    if (st) return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_pointcloud_aabb_mask(const void* points_dev, int64_t n, int dtype,
                               const double min_bound[3],
                               const double max_bound[3],
                               uint8_t* mask_out_dev, int64_t* m_out,
                               o3dmi_stream_t stream) {
    int st = CheckBox(points_dev, n, dtype, mask_out_dev, m_out);
    if (st) return st;
    O3DMI_REQUIRE(min_bound && max_bound, "null argument");
    for (int k = 0; k < 3; ++k)
        O3DMI_REQUIRE(max_bound[k] >= min_bound[k],
                      "max_bound must be >= min_bound on every axis");
    *m_out = 0;
    if (n == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    st = AabbMaskAsync(points_dev, n, dtype, min_bound, max_bound,
                       mask_out_dev, &w->count, s);
    if (st) return st;
    return DownloadCount(w, m_out, s);
}

int o3dmi_pointcloud_obb_mask(const void* points_dev, int64_t n, int dtype,
                              const double center[3], const double rotation[9],
                              const double extent[3], uint8_t* mask_out_dev,
                              int64_t* m_out, o3dmi_stream_t stream) {
    int st = CheckBox(points_dev, n, dtype, mask_out_dev, m_out);
    if (st) return st;
    O3DMI_REQUIRE(center && rotation && extent, "null argument");
    for (int k = 0; k < 3; ++k)
        O3DMI_REQUIRE(extent[k] >= 0, "extent must not be negative");
    *m_out = 0;
    if (n == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    st = ObbMaskAsync(points_dev, n, dtype, center, rotation, extent,
                      mask_out_dev, &w->count, s);
    if (st) return st;
    return DownloadCount(w, m_out, s);
}

int o3dmi_pointcloud_min_max_bound(const void* points_dev, int64_t n,
                                   int dtype, double min_out[3],
                                   double max_out[3], o3dmi_stream_t stream) {
    O3DMI_REQUIRE(min_out && max_out, "null argument");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(n == 0 || points_dev, "null argument");
    for (int k = 0; k < 3; ++k) min_out[k] = max_out[k] = 0;
    if (n == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    double* scratch = nullptr;
    double* result = nullptr;
    int st = pool.Alloc(&scratch, sizeof(double) * MinMaxScratchDoubles());
    if (st) return st;
    st = MinMaxBoundAsync(points_dev, n, dtype, scratch, &result, s);
    if (st) return st;
    double host[6];
    O3DMI_HIP_CHECK(hipMemcpyAsync(host, result, sizeof(host),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) {
        min_out[k] = host[k];
        max_out[k] = host[3 + k];
    }
    return O3DMI_OK;
}

}  // extern "C"
