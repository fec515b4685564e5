// Private header shared by nns.hip (index build + searches), icp.hip (the
// fused search + accumulate kernel), ransac.hip (batched hypothesis scoring)
// and the host drivers: the bucketed uniform grid of the fixed-radius / KNN
// index and its lane-per-query k = 1 search. The wave-per-query search that
// .hip files build their own sinks and output policies on is nns_wave.h.
//
// Index design: cell edge = radius * (1 + 1e-3) (KNN: chosen from the measured
// density). Target points are *reordered* by bucket into 16-byte (32-byte for
// f64) records {x,y,z,original index}, normals likewise, so a query's cell
// visits read contiguous memory instead of chasing a CSR index through 12-byte
// AoS points. A bucket's records are contiguous, but buckets lie in memory in
// the order their ranges were handed out (one wave-aggregated atomic per 64
// buckets) -- no prefix sum over the table: the build is a memset and three
// launches (count, hand out ranges, scatter points + normals) with no scratch
// and nothing to wait for. ranges[b] = {end, count} of bucket b: one 8-byte
// load per visited cell. Nothing a search returns depends on the order in
// memory (every result is defined by (d2, original index)). Cell coordinates are computed in float64 on both the build and
// the query side so that large-offset clouds (1000 m + 5 cm radius, cf.
// cpp/tests/core/NearestNeighborSearch.cpp:831-869) bin consistently.
#pragma once

#include "common.h"

struct o3dmi_nns {
    int dtype = O3DMI_F32;
    int64_t n = 0;
    double radius = 0, inv_cell = 0;
    int64_t n_buckets = 0;
    void* sorted_pts = nullptr;      // Rec4<T>[n]
    void* sorted_normals = nullptr;  // Rec4<T>[n], optional
    uint2* ranges = nullptr;         // [n_buckets + 1] {end, count}; the last
                                     // entry is the build's running total
    double* partials = nullptr;      // [kCUs*4, kNumSums]
    int* tickets = nullptr;          // 9 ticket words of the search launch's
                                     // final-sum tail (icp.hip SumTail), in
                                     // the last row of `partials`; zero
                                     // between launches
};

// Entry points of nns.hip (o3dmi_internal_nns_knn_avg_distance:
// pointcloud_filter.hip) for the host drivers and the other kernels' host
// sides, not in the public header (each is described at its definition).
extern "C" {
int o3dmi_nns_set_normals(o3dmi_nns_t* nns, const void* normals_dev,
                          o3dmi_stream_t stream);
int o3dmi_internal_nns_create_with_normals(
        const void* points_dev, const void* normals_dev, int64_t n, int dtype,
        double radius, o3dmi_stream_t stream, o3dmi_nns_t** out);
int o3dmi_internal_nns_create_many(
        int count, const void* const* points_dev,
        const void* const* normals_dev, const int64_t* n, int dtype,
        const double* radius, o3dmi_stream_t stream, o3dmi_nns_t** out);
int o3dmi_internal_nns_create_small_deferred(
        const void* points_dev, const void* normals_dev, const int* n_dev,
        int dtype, double radius, o3dmi_stream_t stream, o3dmi_nns_t** out);
int o3dmi_internal_nns_adopt_count(o3dmi_nns_t* nns, int64_t n);
int o3dmi_internal_nns_destroy_completed(o3dmi_nns_t* nns);
int o3dmi_internal_nns_hybrid_search_wide(
        const o3dmi_nns_t* nns, const void* queries_dev, const int32_t* ids_dev,
        int64_t nq, int max_knn, int32_t* idx_dev, void* dist2_dev,
        int32_t* counts_dev, o3dmi_stream_t stream);
int o3dmi_nns_knn_search_counts(const void* points_dev, int64_t n,
                                const void* queries_dev, int64_t q, int dtype,
                                int knn, int32_t* idx_dev, void* dist2_dev,
                                int32_t* counts_dev, o3dmi_stream_t stream);
int o3dmi_internal_nns_knn_avg_distance(const void* points_dev, int64_t n,
                                        int dtype, int knn, void* avg_dev,
                                        o3dmi_stream_t stream);
}  // extern "C"

namespace o3dmi {

constexpr int kNumSums = 32;  // 29 + sum d2 + match count + pad

template <typename T> struct Rec4;  // {x,y,z,w}
template <> struct alignas(16) Rec4<float> { float x, y, z; int w; };
template <> struct alignas(32) Rec4<double> { double x, y, z; long long w; };

// 32-bit mixing of the (wrapped) cell coordinates: three multiplies and a
// murmur3 finaliser. (The first version went through 64-bit products and a
// 64-bit finaliser -- five 64-bit multiplies, ~45 vector instructions per
// visited cell, a fifth of the fused ICP search's instruction stream.)
__device__ __forceinline__ unsigned HashCell(long long cx, long long cy,
                                             long long cz) {
    unsigned h = (unsigned)cx * 0x9E3779B1u;
    h ^= ((unsigned)cy * 0x85EBCA77u) + (h >> 15);
    h ^= ((unsigned)cz * 0xC2B2AE3Du) + (h << 11);
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

template <typename T>
__device__ __forceinline__ void CellOf(const T* p, double inv_cell,
                                       long long& cx, long long& cy,
                                       long long& cz) {
    cx = (long long)floor((double)p[0] * inv_cell);
    cy = (long long)floor((double)p[1] * inv_cell);
    cz = (long long)floor((double)p[2] * inv_cell);
}

template <typename T>
__device__ __forceinline__ int RecIndex(const Rec4<T>& r) {
    return (int)r.w;
}

// Gather an {N,3} attribute (normals) into sorted record order.
template <typename T>
struct NnsView {
    const Rec4<T>* sorted;      // [n] bucket-ordered {x,y,z,idx}
    const uint2* ranges;        // [n_buckets] {end, count}
    double inv_cell;
    unsigned mask;
    T radius_squared;
};

// Records of bucket b: sorted[s .. e).
template <typename T>
__device__ __forceinline__ void BucketRange(const NnsView<T>& nv, unsigned b,
                                            unsigned& s, unsigned& e) {
    const uint2 r = nv.ranges[b];
    e = r.x;
    s = r.x - r.y;
}

template <typename T>
inline NnsView<T> MakeView(const o3dmi_nns* nns) {
    NnsView<T> v;
    v.sorted = (const Rec4<T>*)nns->sorted_pts;
    v.ranges = nns->ranges;
    v.inv_cell = nns->inv_cell;
    v.mask = (unsigned)(nns->n_buckets - 1);
    const T r = (T)nns->radius;  // NanoFlannImpl.h:332: T radius_squared
    v.radius_squared = r * r;
    return v;
}

// The square root every distance output takes, in the point dtype (float32:
// correctly rounded under the library's build flags).
__device__ __forceinline__ float SqrtOf(float x) { return sqrtf(x); }
__device__ __forceinline__ double SqrtOf(double x) { return sqrt(x); }

// One level of the KNN index (nns_wave.h, "k nearest neighbours without a
// radius"): the bucketed grid, its cell edge and the occupied cell box.
template <typename T>
struct KnnGrid {
    NnsView<T> nv;
    double cell;
    long long cmin[3], cmax[3];  // occupied cell box
};

// Shells a level is searched for before a query is left to a coarser one.
constexpr int kKnnShells = 3;

template <typename T>
inline KnnGrid<T> MakeKnnGrid(const o3dmi_nns* lv, const long long* cmin,
                              const long long* cmax) {
    KnnGrid<T> g;
    g.nv = MakeView<T>(lv);
    g.cell = lv->radius;
    for (int a = 0; a < 3; ++a) {
        g.cmin[a] = cmin[a];
        g.cmax[a] = cmax[a];
    }
    return g;
}

// Nearest neighbour with d2 < r2 (strict), ties -> lowest original index.
// Returns the position in the sorted array (or -1); idx/d2 by reference.
// Distance arithmetic: nanoflann::L2_Adaptor::evalMetric for dim 3,
// ((dx*dx) + dy*dy) + dz*dz with dx = query - point, in T.
template <typename T>
__device__ __forceinline__ int SearchNearest(const NnsView<T>& nv, const T* q,
                                             int& best_idx, T& best_d2) {
    long long cx, cy, cz;
    CellOf(q, nv.inv_cell, cx, cy, cz);
    int best_pos = -1;
    best_idx = -1;
    best_d2 = 0;
    const T qx = q[0], qy = q[1], qz = q[2];
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                unsigned b = HashCell(cx + dx, cy + dy, cz + dz) & nv.mask;
                unsigned s, e;
                BucketRange(nv, b, s, e);
                for (unsigned j = s; j < e; ++j) {
                    Rec4<T> p = nv.sorted[j];
                    T result = T(0);
                    const T d0 = qx - p.x;
                    result += d0 * d0;
                    const T d1 = qy - p.y;
                    result += d1 * d1;
                    const T d2 = qz - p.z;
                    result += d2 * d2;
                    if (result < nv.radius_squared) {
                        int idx = RecIndex(p);
                        if (best_pos < 0 || result < best_d2 ||
                            (result == best_d2 && idx < best_idx)) {
                            best_pos = (int)j;
                            best_idx = idx;
                            best_d2 = result;
                        }
                    }
                }
            }
    return best_pos;
}

}  // namespace o3dmi
