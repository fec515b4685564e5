// t::pipelines::registration::ComputeFPFHFeature and
// CorrespondencesFromFeatures (t/pipelines/registration/Feature.cpp:23-333)
// over the kernels of feature.hip and the grid index of nns.hip.
//
// Neighbour lists, as the reference's three modes:
//   hybrid (radius + max_nn): the grid index's HybridSearch, up to 128 per row;
//   KNN (max_nn only): k = min(max_nn, N) nearest by (d2, index). A hybrid
//     search within a radius R is the exact KNN list of every row that finds
//     k points (any point left out lies at d2 >= R^2); rows that find fewer
//     are searched again with 2R until none is left (R > the cloud's diagonal
//     finds every point);
//   radius only: CSR lists from the fixed-radius search.
// With `indices`, rows follow NonZero(mask) of the indices, as the reference;
// lists and SPFH rows are computed for the requested points and their
// neighbours only.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "feature.h"
#include "nns.h"
#include "o3d_mi355x_host.h"
#include "scan.h"

using namespace o3dmi;

namespace {

constexpr int kMaxFpfhNn = 128;

// The scratch and search indices of one call; released once the stream has
// drained.
struct SearchScratch : PoolScratch {
    std::vector<o3dmi_nns_t*> indices;
    explicit SearchScratch(hipStream_t st) : PoolScratch(st) {}
    ~SearchScratch() {
        (void)hipStreamSynchronize(s);
        for (o3dmi_nns_t* x : indices) o3dmi_nns_destroy(x);
    }
    int Index(const void* pts, int64_t n, int dtype, double radius,
              o3dmi_nns_t** out) {
        const int st = o3dmi_nns_create(pts, n, dtype, radius,
                                        (o3dmi_stream_t)s, out);
        if (!st) indices.push_back(*out);
        return st;
    }
};

// Neighbour lists of nq query positions: padded {nq, width} + counts, or CSR.
struct NbLists {
    int32_t* idx = nullptr;
    void* d2 = nullptr;
    int32_t* counts = nullptr;
    int64_t* splits = nullptr;
    int width = 0;
    int64_t entries = 0;  // idx entries (padded: nq * width)
};

struct Search {
    const void* pts;
    int64_t n;
    int dtype;
    size_t esz;
    int max_nn;      // <= 0: none
    double radius;   // <= 0: none
    o3dmi_nns_t* index = nullptr;  // hybrid / radius
    double diag = 0, knn_r0 = 0;   // KNN

    int Prepare(SearchScratch& sc) {
        if (radius > 0) return sc.Index(pts, n, dtype, radius, &index);
        double lo[3], hi[3];
        int st = o3dmi_internal_bounds(pts, n, dtype, lo, hi,
                                       (o3dmi_stream_t)sc.s);
        if (st) return st;
        double e[3];
        for (int a = 0; a < 3; ++a) e[a] = std::max(hi[a] - lo[a], 0.0);
        diag = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        std::sort(e, e + 3);
        const int k = (int)std::min<int64_t>(max_nn, n);
        // k points within R on a surface spanning the two largest extents, in
        // a filled box, or on a line: the largest of the three guesses
        const double pi = 3.14159265358979323846;
        double r = std::sqrt(e[2] * e[1] * k / (pi * (double)n));
        r = std::max(r, std::cbrt(e[0] * e[1] * e[2] * k * 0.75 /
                                  (pi * (double)n)));
        r = std::max(r, e[2] * k * 0.5 / (double)n);
        r *= 1.25;
        if (!(r > diag * 1e-6)) r = diag * 1e-6;
        if (!(r > 0)) r = 1.0;
        knn_r0 = r;
        return O3DMI_OK;
    }

    int Run(SearchScratch& sc, const void* q, int64_t nq, NbLists* out) {
        o3dmi_stream_t stream = (o3dmi_stream_t)sc.s;
        int st;
        if (radius > 0 && max_nn <= 0) {
            // FixedRadiusSearch: CSR
            int32_t* cnt = nullptr;
            void* tmp = nullptr;
            if ((st = sc.Alloc(&cnt, 4 * (size_t)nq)) ||
                (st = sc.Alloc(&out->splits, 8 * (size_t)(nq + 1))) ||
                (st = sc.Alloc(&tmp, ScanScratchBytes(nq))))
                return st;
            O3DMI_HIP_CHECK(hipMemsetAsync(out->splits, 0, 8, sc.s));
            if (nq > 0) {
                if ((st = o3dmi_nns_radius_count(index, q, nq, cnt, stream)))
                    return st;
                if ((st = PrefixSumAsync(cnt, nq, true, out->splits + 1,
                                         nullptr, tmp, sc.s)))
                    return st;
            }
            O3DMI_HIP_CHECK(hipMemcpyAsync(&out->entries, out->splits + nq, 8,
                                           hipMemcpyDeviceToHost, sc.s));
            O3DMI_HIP_CHECK(hipStreamSynchronize(sc.s));
            if ((st = sc.Alloc(&out->idx, 4 * (size_t)out->entries)) ||
                (st = sc.Alloc(&out->d2, esz * (size_t)out->entries)))
                return st;
            return nq > 0 ? o3dmi_nns_radius_search(index, q, nq, out->splits,
                                                    out->idx, out->d2, stream)
                          : O3DMI_OK;
        }
        const int width =
                radius > 0 ? max_nn : (int)std::min<int64_t>(max_nn, n);
        out->width = width;
        out->entries = nq * width;
        if ((st = sc.Alloc(&out->idx, 4 * (size_t)out->entries)) ||
            (st = sc.Alloc(&out->d2, esz * (size_t)out->entries)) ||
            (st = sc.Alloc(&out->counts, 4 * (size_t)nq)))
            return st;
        if (nq == 0) return O3DMI_OK;
        if (radius > 0)  // HybridSearch
            return o3dmi_internal_nns_hybrid_search_wide(
                    index, q, nullptr, nq, max_nn, out->idx, out->d2,
                    out->counts, stream);
        // KnnSearch through hybrid searches of growing radius
        int32_t* ids = nullptr;
        int* n_ids_dev = nullptr;
        if ((st = sc.Alloc(&ids, 4 * (size_t)nq)) ||
            (st = sc.Alloc(&n_ids_dev, sizeof(int))))
            return st;
        double r = knn_r0;
        const int32_t* rows = nullptr;
        int64_t n_rows = nq;
        for (int round = 0; n_rows > 0; ++round) {
            // past the diagonal every point is within reach: a few dozen
            // doublings at most
            if (round >= 60) {
                SetLastError("KNN search did not converge");
                return O3DMI_ERR_INTERNAL;
            }
            o3dmi_nns_t* idx = nullptr;
            if ((st = o3dmi_nns_create(pts, n, dtype, r, stream, &idx)))
                return st;
            st = o3dmi_internal_nns_hybrid_search_wide(
                    idx, q, rows, n_rows, width, out->idx, out->d2,
                    out->counts, stream);
            int short_rows = 0;
            if (!st)
                st = o3dmi_internal_short_rows(out->counts, nq, width, ids,
                                               n_ids_dev, &short_rows, stream);
            // this round's index is released now, not at the end of the call
            // (short_rows has waited for the search; on an error, drain first)
            if (st) (void)hipStreamSynchronize(sc.s);
            o3dmi_internal_nns_destroy_completed(idx);
            if (st) return st;
            rows = ids;
            n_rows = short_rows;
            r *= 2.0;
        }
        return O3DMI_OK;
    }
};

template <typename T>
int Gather(const void* pts, const int32_t* list, int64_t m, void* out,
           hipStream_t s) {
    return GatherRows(pts, (const int*)list, m, 3 * sizeof(T), out, s);
}

}  // namespace

extern "C" {

int o3dmi_registration_compute_fpfh_feature(
        const void* points_dev, const void* normals_dev, int64_t n, int dtype,
        int has_max_nn, int max_nn, int has_radius, double radius,
        const int64_t* indices_dev, int64_t n_indices, void* fpfhs_dev,
        int64_t* n_rows_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(!has_max_nn || max_nn > 3, "max_nn must be greater than 3.");
    O3DMI_REQUIRE(!has_radius || radius > 0, "radius must be greater than 0.");
    O3DMI_REQUIRE(normals_dev != nullptr, "The input point cloud has no normal.");
    O3DMI_REQUIRE(has_max_nn || has_radius, "Both max_nn and radius are none.");
    O3DMI_REQUIRE(n_rows_out != nullptr, "n_rows_out is null");
    // the grid index addresses its records by 32-bit byte offsets (32 B per
    // Float64 record): o3dmi_nns_create takes fewer than 2^27 points
    O3DMI_REQUIRE(n >= 0 && n < (1ll << 27), "n out of range (< 2^27 points)");
    if (has_max_nn && max_nn > kMaxFpfhNn) {
        SetLastError("max_nn > 128 is not supported");
        return O3DMI_ERR_UNSUPPORTED;
    }
    *n_rows_out = 0;
    O3DMI_REQUIRE(n_indices <= 0 || indices_dev != nullptr, "indices is null");
    const bool filter = indices_dev != nullptr || n_indices >= 0;
    if (filter && n_indices <= 0) return O3DMI_OK;  // Zeros({0, 33})
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(points_dev && fpfhs_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t esz = dtype == O3DMI_F64 ? 8 : 4;
    SearchScratch sc(s);
    Search search{points_dev, n, dtype, esz, has_max_nn ? max_nn : 0,
                  has_radius ? radius : 0.0};
    int st = search.Prepare(sc);
    if (st) return st;
    if (!filter) {
        NbLists l;
        if ((st = search.Run(sc, points_dev, n, &l))) return st;
        if ((st = o3dmi_fpfh_from_neighbors(
                     points_dev, normals_dev, n, dtype, l.idx, l.d2, l.counts,
                     l.splits, l.width, n, nullptr, nullptr, fpfhs_dev,
                     n_rows_out, stream)))
            return st;
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        return O3DMI_OK;
    }
    // the requested points: mask, NonZero
    uint8_t* mask = nullptr;
    uint8_t* need = nullptr;
    int* bad = nullptr;
    int32_t* list = nullptr;
    int64_t* rows64 = nullptr;
    void* qpos = nullptr;
    if ((st = sc.Alloc(&mask, (size_t)n)) ||
        (st = sc.Alloc(&need, (size_t)n)) ||
        (st = sc.Alloc(&bad, sizeof(int))) ||
        (st = sc.Alloc(&list, 4 * (size_t)n)) ||
        (st = sc.Alloc(&rows64, 8 * (size_t)n)) ||
        (st = sc.Alloc(&qpos, 3 * esz * (size_t)n)))
        return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(mask, 0, (size_t)n, s));
    O3DMI_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), s));
    if ((st = o3dmi_internal_fpfh_mark_indices(indices_dev, n_indices, n, mask,
                                               bad, stream)))
        return st;
    int hbad = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&hbad, bad, sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    O3DMI_REQUIRE(!hbad, "indices out of range");
    int64_t n_req = 0;
    if ((st = o3dmi_internal_mask_nonzero(mask, n, list, nullptr, &n_req,
                                          stream)))
        return st;
    // their neighbours: every point whose SPFH the requested rows read
    const int gs = dtype == O3DMI_F64 ? Gather<double>(points_dev, list, n_req,
                                                       qpos, s)
                                      : Gather<float>(points_dev, list, n_req,
                                                      qpos, s);
    if (gs) return gs;
    {
        NbLists l1;
        if ((st = search.Run(sc, qpos, n_req, &l1))) return st;
        O3DMI_HIP_CHECK(hipMemcpyAsync(need, mask, (size_t)n,
                                       hipMemcpyDeviceToDevice, s));
        if ((st = o3dmi_internal_fpfh_mark_lists(l1.idx, l1.entries, need,
                                                 stream)))
            return st;
    }
    int64_t n_spfh = 0;
    if ((st = o3dmi_internal_mask_nonzero(need, n, list, rows64, &n_spfh,
                                          stream)))
        return st;
    const int gs2 = dtype == O3DMI_F64 ? Gather<double>(points_dev, list,
                                                        n_spfh, qpos, s)
                                       : Gather<float>(points_dev, list,
                                                       n_spfh, qpos, s);
    if (gs2) return gs2;
    NbLists l;
    if ((st = search.Run(sc, qpos, n_spfh, &l))) return st;
    if ((st = o3dmi_fpfh_from_neighbors(points_dev, normals_dev, n, dtype,
                                        l.idx, l.d2, l.counts, l.splits,
                                        l.width, n_spfh, mask, rows64,
                                        fpfhs_dev, n_rows_out, stream)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_registration_correspondences_from_features(
        const void* source_dev, int64_t n_source, const void* target_dev,
        int64_t n_target, int dim, int dtype, int mutual_filter,
        float mutual_consistency_ratio, int64_t* correspondences_dev,
        int64_t* n_correspondences, int* fell_back, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n_correspondences != nullptr, "n_correspondences is null");
    O3DMI_REQUIRE(n_source >= 0 && n_target > 0, "empty feature set");
    hipStream_t s = (hipStream_t)stream;
    *n_correspondences = 0;
    if (fell_back) *fell_back = 0;
    if (n_source == 0) return O3DMI_OK;
    O3DMI_REQUIRE(correspondences_dev != nullptr, "correspondences is null");
    SearchScratch sc(s);
    int32_t* ij = nullptr;
    int32_t* ji = nullptr;
    int64_t* info = nullptr;
    int st;
    if ((st = sc.Alloc(&ij, 4 * (size_t)n_source)) ||
        (st = sc.Alloc(&info, 16)))
        return st;
    if ((st = o3dmi_internal_feature_nn1(source_dev, n_source, target_dev,
                                         n_target, dim, dtype, ij, stream)))
        return st;
    if (mutual_filter) {
        if ((st = sc.Alloc(&ji, 4 * (size_t)n_target))) return st;
        if ((st = o3dmi_internal_feature_nn1(target_dev, n_target, source_dev,
                                             n_source, dim, dtype, ji,
                                             stream)))
            return st;
    }
    if ((st = o3dmi_internal_feature_mutual(ij, ji, n_source,
                                            mutual_filter ? 1 : 0,
                                            mutual_consistency_ratio,
                                            correspondences_dev, info,
                                            stream)))
        return st;
    int64_t h[2];
    O3DMI_HIP_CHECK(hipMemcpyAsync(h, info, sizeof(h), hipMemcpyDeviceToHost,
                                   s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    *n_correspondences = h[0];
    if (fell_back) *fell_back = (int)h[1];
    return O3DMI_OK;
}

}  // extern "C"
