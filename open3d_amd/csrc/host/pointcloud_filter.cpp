// Host drivers of the PointCloud selection and filter family
// (t/geometry/PointCloud.cpp:435-494, 650-760) and of
// slac::PreprocessPointClouds' per-fragment step (t/pipelines/slac/
// SLACOptimizer.cpp:25-64). Arguments are checked before anything is
// allocated or launched; the kernels are in pointcloud_filter.hip, the
// radius count in nns.hip.
#include <cmath>

#include "../pointcloud_filter.h"
#include "o3d_mi355x_host.h"
#include "pointcloud_call.h"

using namespace o3dmi;

namespace {

constexpr int kMaxFilterKnn = 64;  // one wave's list (nns_wave.h kMaxKnn)

int SelectByMaskImpl(int64_t n, const uint8_t* mask_dev, bool invert,
                     const SelectAttrs& attrs, int64_t* m_out, hipStream_t s) {
    PoolScratch pool(s);
    char* scratch = nullptr;
    Words* w = nullptr;  // not zeroed: the compaction stores the count
    int st = pool.Alloc(&scratch, CompactScratchBytes(n));
    if (!st) st = pool.Alloc(&w, 256);
    if (st) return st;
    st = CompactByMaskAsync(mask_dev, n, invert, attrs, (int64_t*)&w->count,
                            scratch, s);
    if (st) return st;
    return DownloadCount(w, m_out, s);
}

}  // namespace

extern "C" {

int o3dmi_pointcloud_select_by_mask(int64_t n, const uint8_t* mask_dev,
                                    int invert, int n_attrs,
                                    const void* const* attrs_in,
                                    const int64_t* row_bytes,
                                    void* const* attrs_out, int64_t* m_out,
                                    o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    SelectAttrs attrs;
    int st = CheckAttrs(n_attrs, attrs_in, row_bytes, attrs_out, n > 0, &attrs);
    if (st) return st;
    O3DMI_REQUIRE(n == 0 || mask_dev, "mask is null");
    *m_out = 0;
    if (n == 0) return O3DMI_OK;
    return SelectByMaskImpl(n, mask_dev, invert != 0, attrs, m_out,
                            (hipStream_t)stream);
}

int o3dmi_pointcloud_select_by_index(int64_t n, const int64_t* indices_dev,
                                     int64_t m, int invert,
                                     int remove_duplicates, int n_attrs,
                                     const void* const* attrs_in,
                                     const int64_t* row_bytes,
                                     void* const* attrs_out, int64_t* m_out,
                                     o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0 && m >= 0, "n < 0 or m < 0");
    const bool by_mask = invert || remove_duplicates;
    SelectAttrs attrs;
    int st = CheckAttrs(n_attrs, attrs_in, row_bytes, attrs_out,
                        by_mask ? n > 0 : m > 0, &attrs);
    if (st) return st;
    O3DMI_REQUIRE(m == 0 || indices_dev, "indices is null");
    *m_out = 0;
    if (m == 0 && (!invert || n == 0)) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = CheckIndexRangeAsync(indices_dev, m, n, &w->bad, s))) return st;
    int bad = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&bad, &w->bad, sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    O3DMI_REQUIRE(!bad, "select_by_index: index outside [0, n)");
    if (!by_mask) {
        if ((st = GatherByIndexAsync(indices_dev, m, attrs, s))) return st;
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        *m_out = m;
        return O3DMI_OK;
    }
    // upstream: mask = zeros; mask[indices] = true; SelectByMask(mask, invert)
    uint8_t* mask = nullptr;
    if ((st = pool.Alloc(&mask, (size_t)n))) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(mask, 0, (size_t)n, s));
    if ((st = IndexToMaskAsync(indices_dev, m, mask, s))) return st;
    return SelectByMaskImpl(n, mask, invert != 0, attrs, m_out, s);
}

int o3dmi_pointcloud_remove_non_finite_points(const void* points_dev,
                                              int64_t n, int dtype,
                                              int remove_nan, int remove_inf,
                                              uint8_t* mask_out_dev,
                                              int64_t* m_out,
                                              o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(n == 0 || (points_dev && mask_out_dev), "null argument");
    *m_out = 0;
    if (n == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    int st = AllocWords(pool, &w);
    if (st) return st;
    st = NonFiniteMaskAsync(points_dev, n, dtype, remove_nan != 0,
                            remove_inf != 0, mask_out_dev, &w->count, s);
    if (st) return st;
    return DownloadCount(w, m_out, s);
}

int o3dmi_pointcloud_remove_duplicated_points(const void* points_dev,
                                              int64_t n, int dtype,
                                              uint8_t* mask_out_dev,
                                              int64_t* m_out,
                                              o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(n == 0 || (points_dev && mask_out_dev), "null argument");
    O3DMI_REQUIRE(n < (1ll << 30), "too many points (< 2^30)");
    *m_out = 0;
    if (n == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    int32_t* table = nullptr;
    const int64_t slots = DuplicateTableSlots(n);
    int st = AllocWords(pool, &w);
    if (!st) st = pool.Alloc(&table, sizeof(int32_t) * (size_t)slots);
    if (st) return st;
    st = DuplicateMaskAsync(points_dev, n, dtype, table, slots, mask_out_dev,
                            &w->count, s);
    if (st) return st;
    return DownloadCount(w, m_out, s);
}

int o3dmi_pointcloud_remove_radius_outliers(const void* points_dev, int64_t n,
                                            int dtype, int64_t nb_points,
                                            double search_radius,
                                            uint8_t* mask_out_dev,
                                            int64_t* m_out,
                                            o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(nb_points >= 1 && search_radius > 0,
                  "Illegal input parameters, number of points and radius must "
                  "be positive");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(n == 0 || (points_dev && mask_out_dev), "null argument");
    O3DMI_REQUIRE(n < (1ll << 27), "n out of range (< 2^27 points)");
    *m_out = 0;
    if (n == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    int32_t* counts = nullptr;
    int st = AllocWords(pool, &w);
    if (!st) st = pool.Alloc(&counts, sizeof(int32_t) * (size_t)n);
    if (st) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    NnsGuard index;
    st = o3dmi_nns_create(points_dev, n, dtype, search_radius, stream,
                          &index.nns);
    if (st) return st;
    st = o3dmi_nns_radius_count(index.nns, points_dev, n, counts, stream);
    if (st) return st;
    // a count never exceeds n < 2^27
    const int need = nb_points > n ? (int)(n + 1) : (int)nb_points;
    st = CountThresholdMaskAsync(counts, n, need, mask_out_dev, &w->count, s);
    if (st) return st;
    st = DownloadCount(w, m_out, s);
    index.completed = st == O3DMI_OK;  // the stream has drained
    return st;
}

int o3dmi_pointcloud_remove_statistical_outliers(
        const void* points_dev, int64_t n, int dtype, int64_t nb_neighbors,
        double std_ratio, uint8_t* mask_out_dev, void* avg_distances_out_dev,
        double* stats_out, int64_t* m_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(nb_neighbors >= 1 && std_ratio > 0,
                  "Illegal input parameters, the number of neighbors and "
                  "standard deviation ratio must be positive.");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(n == 0 || (points_dev && mask_out_dev), "null argument");
    if (nb_neighbors > kMaxFilterKnn)
        return Unsupported("nb_neighbors > 64 is not supported");
    O3DMI_REQUIRE(n < (1ll << 31) - 1, "too many points");
    *m_out = 0;
    if (n == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    double* sums = nullptr;
    double* stats = nullptr;  // {mean, std, threshold, count}
    void* avg = avg_distances_out_dev;
    int st = AllocWords(pool, &w);
    if (!st) st = pool.Alloc(&sums, sizeof(double) * StatisticalScratchDoubles());
    if (!st) st = pool.Alloc(&stats, 256);
    if (!st && !avg) st = pool.Alloc(&avg, ElemSize(dtype) * (size_t)n);
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(stats, 0, 32, s));
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    st = o3dmi_internal_nns_knn_avg_distance(points_dev, n, dtype,
                                             (int)nb_neighbors, avg, stream);
    if (st) return st;
    st = StatisticalMaskAsync(avg, n, dtype, std_ratio, sums, stats,
                              mask_out_dev, s);
    if (st) return st;
    double host[4];
    O3DMI_HIP_CHECK(hipMemcpyAsync(host, stats, sizeof(host),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    if (stats_out)
        for (int k = 0; k < 3; ++k) stats_out[k] = host[k];
    unsigned long long c;
    std::memcpy(&c, &host[3], sizeof(c));
    *m_out = (int64_t)c;
    return O3DMI_OK;
}

int o3dmi_slac_preprocess_point_cloud(const void* points_dev,
                                      const void* normals_dev, int64_t n,
                                      int dtype, double voxel_size,
                                      int apply_outlier_mask,
                                      void* out_points_dev,
                                      void* out_normals_dev, int64_t* m_out,
                                      o3dmi_stream_t stream) {
    O3DMI_REQUIRE(m_out != nullptr, "m_out is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(n == 0 || (points_dev && out_points_dev && out_normals_dev),
                  "null argument");
    *m_out = 0;
    if (n == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t row = 3 * ElemSize(dtype);
    const bool down = voxel_size > 0;
    PoolScratch pool(s);
    uint8_t* mask = nullptr;
    char* stage_p = nullptr;  // the cloud before the filter is applied
    char* stage_n = nullptr;
    int st = pool.Alloc(&mask, (size_t)n);
    if (!st && apply_outlier_mask) st = pool.Alloc(&stage_p, row * (size_t)n);
    if (!st && apply_outlier_mask && normals_dev)
        st = pool.Alloc(&stage_n, row * (size_t)n);
    if (st) return st;
    void* cur_p = apply_outlier_mask ? (void*)stage_p : out_points_dev;
    void* cur_n = normals_dev
                          ? (apply_outlier_mask ? (void*)stage_n
                                                : out_normals_dev)
                          : nullptr;
    int64_t m = n;
    if (down) {
        st = o3dmi_voxel_down_sample(points_dev, normals_dev, n, dtype,
                                     voxel_size, cur_p, cur_n, &m, stream);
        if (st) return st;
    } else {
        O3DMI_HIP_CHECK(hipMemcpyAsync(cur_p, points_dev, row * (size_t)n,
                                       hipMemcpyDeviceToDevice, s));
        if (normals_dev)
            O3DMI_HIP_CHECK(hipMemcpyAsync(cur_n, normals_dev, row * (size_t)n,
                                           hipMemcpyDeviceToDevice, s));
    }
    // upstream computes the filter in both branches and drops what it returns
    int64_t kept = 0;
    st = o3dmi_pointcloud_remove_statistical_outliers(
            cur_p, m, dtype, 20, 2.0, mask, nullptr, nullptr, &kept, stream);
    if (st) return st;
    if (apply_outlier_mask) {
        SelectAttrs attrs;
        attrs.n_attrs = cur_n ? 2 : 1;
        attrs.in[0] = cur_p;
        attrs.out[0] = out_points_dev;
        attrs.row_bytes[0] = (long long)row;
        attrs.in[1] = cur_n;
        attrs.out[1] = out_normals_dev;
        attrs.row_bytes[1] = (long long)row;
        if ((st = SelectByMaskImpl(m, mask, false, attrs, &m, s))) return st;
    }
    // down-sampled clouds always get fresh normals (oriented like the averaged
    // ones when normals came in); others only when none came
    if (down || !normals_dev) {
        st = o3dmi_pointcloud_estimate_normals(out_points_dev, m, dtype, 30,
                                               -1.0, out_normals_dev,
                                               normals_dev ? 1 : 0, stream);
        if (st) return st;
    }
    *m_out = m;
    return O3DMI_OK;
}

}  // extern "C"
