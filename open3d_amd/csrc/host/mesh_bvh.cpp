// Host drivers of the closest-point queries on a triangle mesh
// (RaycastingScene::ComputeClosestPoints / ComputeDistance for one triangle
// geometry, t/geometry/RaycastingScene.cpp:1464-1517) and of
// TriangleMesh::ComputeMetrics (t/geometry/TriangleMesh.cpp:1939-1967).
// Arguments are checked before anything is allocated, the triangle indices
// and the coordinates on the device before anything is written; the kernels
// are in mesh_bvh.hip.
#include <algorithm>
#include <memory>
#include <vector>

#include "../mesh_bvh.h"
#include "../pointcloud_metrics.h"
#include "o3d_mi355x_host.h"
#include "trianglemesh_call.h"

using namespace o3dmi;

namespace {

int CheckSceneFloat(int dtype, const char* what) {
    if (dtype == O3DMI_F64)
        return Unsupported("closest points: Float32 only (upstream's scene)");
    O3DMI_REQUIRE(dtype == O3DMI_F32, what);
    return O3DMI_OK;
}

void FreeBvh(o3dmi_mesh_bvh* b) {
    if (!b) return;
    PoolFree(b->nodes);
    PoolFree(b->leaves);
    delete b;
}

struct BvhDeleter {
    void operator()(o3dmi_mesh_bvh* b) const { FreeBvh(b); }
};
using BvhPtr = std::unique_ptr<o3dmi_mesh_bvh, BvhDeleter>;

// The arguments of a mesh a scene is built from.
int CheckSceneMesh(const void* positions_dev, int64_t v, int dtype,
                   const void* triangles_dev, int64_t m, int index_dtype) {
    int st = CheckSceneFloat(dtype, "positions must be Float32");
    if (!st) st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(m > 0, "the mesh has no triangles");
    O3DMI_REQUIRE(positions_dev && triangles_dev, "null argument");
    return O3DMI_OK;
}

// Builds the handle of a mesh whose arguments CheckSceneMesh accepted. Waits
// for the build: the handle is complete on return.
int CreateBvh(const void* positions_dev, int64_t v, const void* triangles_dev,
              int64_t m, int index_dtype, BvhPtr* out, hipStream_t s) {
    BvhPtr bvh(new o3dmi_mesh_bvh);
    {
        PoolScratch pool(s);
        Words* w = nullptr;
        const int32_t* tri = nullptr;
        void* scratch = nullptr;
        float* scene = nullptr;
        int st = AllocWords(pool, &w);
        if (st) return st;
        if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v,
                                &tri)))
            return st;
        if ((st = RequireFinite(positions_dev, v, O3DMI_F32, w, s))) return st;
        if ((st = pool.Alloc(&scratch, MeshBvhBuildScratchBytes(m)))) return st;
        if ((st = pool.Alloc(&scene, 256))) return st;
        void* p = nullptr;
        if (m > 1) {
            if ((st = PoolAlloc(&p, sizeof(BvhNode) * (size_t)(m - 1))))
                return st;
            bvh->nodes = (BvhNode*)p;
        }
        if ((st = PoolAlloc(&p, sizeof(BvhLeaf) * (size_t)m))) return st;
        bvh->leaves = (BvhLeaf*)p;
        bvh->m = m;
        if ((st = BuildMeshBvhAsync((const float*)positions_dev, tri, m,
                                    bvh->nodes, bvh->leaves, scene, scratch,
                                    s)))
            return st;
        O3DMI_HIP_CHECK(hipMemcpyAsync(bvh->scene, scene, 6 * sizeof(float),
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    }
    *out = std::move(bvh);
    return O3DMI_OK;
}

MeshBvhView ViewOf(const o3dmi_mesh_bvh* b) {
    MeshBvhView view;
    view.nodes = b->nodes;
    view.leaves = b->leaves;
    view.m = b->m;
    for (int k = 0; k < 3; ++k) {
        view.scene_lo[k] = b->scene[k];
        view.scene_hi[k] = b->scene[3 + k];
    }
    return view;
}

// Whether the lanes take the queries in Morton order. Measured:
// the sort costs more than it saves at 100 k queries and wins a few per cent
// at 1 M, so the simpler input order is kept.
constexpr bool kSortQueries = false;

int CheckQueries(const void* queries_dev, int64_t q, int dtype) {
    O3DMI_REQUIRE(q >= 0 && q < (1ll << 31) - 1, "q out of range");
    const int st = CheckSceneFloat(dtype, "queries must be Float32");
    if (st) return st;
    O3DMI_REQUIRE(q == 0 || queries_dev, "null argument");
    return O3DMI_OK;
}

// Checked queries (q > 0) against a complete handle. Waits.
int RunQuery(const o3dmi_mesh_bvh* bvh, const void* queries_dev, int64_t q,
             const MeshQueryOut& out, bool sort_queries,
             unsigned long long* visits_out, hipStream_t s) {
    PoolScratch pool(s);
    Words* w = nullptr;
    unsigned long long* visits = nullptr;
    void* scratch = nullptr;
    int st = AllocWords(pool, &w);
    if (st) return st;
    if ((st = RequireFinite(queries_dev, q, O3DMI_F32, w, s))) return st;
    if (visits_out) {
        if ((st = pool.Alloc(&visits, 256))) return st;
        O3DMI_HIP_CHECK(hipMemsetAsync(visits, 0, 16, s));
    }
    if (sort_queries &&
        (st = pool.Alloc(&scratch, MeshBvhQueryScratchBytes(q))))
        return st;
    // w->bad is still zero: RequireFinite passed
    if ((st = MeshBvhQueryAsync(ViewOf(bvh), (const float*)queries_dev, q, out,
                                sort_queries, scratch, &w->bad, visits, s)))
        return st;
    int overflow = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&overflow, &w->bad, sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    if (visits_out)
        O3DMI_HIP_CHECK(hipMemcpyAsync(visits_out, visits, 16,
                                       hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    if (overflow) {
        SetLastError("closest points: traversal stack overflow");
        return O3DMI_ERR_INTERNAL;
    }
    return O3DMI_OK;
}

MeshQueryOut Outputs(void* points, uint32_t* ids, void* uvs, void* normals,
                     void* distance) {
    MeshQueryOut out = {};
    out.points = (float*)points;
    out.ids = ids;
    out.uvs = (float*)uvs;
    out.normals = (float*)normals;
    out.distance = (float*)distance;
    return out;
}

// What one direction of ComputeMetrics leaves on the host.
struct Direction {
    double sum = 0, max = 0;
    std::vector<int64_t> counts;
};

// The d2 of `samples` against `bvh` and their reduction, as for clouds.
int RunDirection(const o3dmi_mesh_bvh* bvh, const float* samples_dev,
                 int64_t q, const float* radii, int n_radii, Direction* dir,
                 hipStream_t s) {
    PoolScratch pool(s);
    const int groups = std::max(
            1, (n_radii + kMetricsRadiusGroup - 1) / kMetricsRadiusGroup);
    float* d2 = nullptr;
    MetricsWords* words = nullptr;
    double* sums = nullptr;
    int st = pool.Alloc(&d2, sizeof(float) * (size_t)q);
    if (!st) st = pool.Alloc(&words, sizeof(MetricsWords) * (size_t)groups);
    if (!st)
        st = pool.Alloc(&sums, sizeof(double) * MetricsSumScratchDoubles(q));
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(words, 0,
                                   sizeof(MetricsWords) * (size_t)groups, s));
    MeshQueryOut out = {};
    out.d2 = d2;
    if ((st = RunQuery(bvh, samples_dev, q, out, kSortQueries, nullptr, s)))
        return st;
    const double* total = nullptr;
    for (int g = 0; g < groups; ++g) {
        const int first = g * kMetricsRadiusGroup;
        const int count = std::min(kMetricsRadiusGroup, n_radii - first);
        st = MetricsReduceAsync(d2, q, O3DMI_F32, nullptr, radii + first,
                                count > 0 ? count : 0, g == 0, words + g, sums,
                                &total, s);
        if (st) return st;
    }
    std::vector<MetricsWords> host((size_t)groups);
    O3DMI_HIP_CHECK(hipMemcpyAsync(host.data(), words,
                                   sizeof(MetricsWords) * (size_t)groups,
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipMemcpyAsync(&dir->sum, total, sizeof(double),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    std::memcpy(&dir->max, &host[0].max_bits, sizeof(double));
    dir->counts.resize((size_t)n_radii);
    for (int r = 0; r < n_radii; ++r)
        dir->counts[(size_t)r] = (int64_t)host[(size_t)(r / kMetricsRadiusGroup)]
                                         .counts[r % kMetricsRadiusGroup];
    return O3DMI_OK;
}

}  // namespace

extern "C" {

int o3dmi_mesh_bvh_create(const void* positions_dev, int64_t v, int dtype,
                          const void* triangles_dev, int64_t m,
                          int index_dtype, o3dmi_mesh_bvh_t** bvh_out,
                          o3dmi_stream_t stream) {
    O3DMI_REQUIRE(bvh_out, "null argument");
    int st = CheckSceneMesh(positions_dev, v, dtype, triangles_dev, m,
                            index_dtype);
    if (st) return st;
    BvhPtr bvh;
    if ((st = CreateBvh(positions_dev, v, triangles_dev, m, index_dtype, &bvh,
                        (hipStream_t)stream)))
        return st;
    *bvh_out = bvh.release();
    return O3DMI_OK;
}

int o3dmi_mesh_bvh_destroy(o3dmi_mesh_bvh_t* bvh) {
    if (!bvh) return O3DMI_OK;
    // queries wait before they return; a caller's own stream work on the
    // outputs does not touch the handle
    FreeBvh(bvh);
    return O3DMI_OK;
}

int o3dmi_internal_mesh_bvh_query(const o3dmi_mesh_bvh* bvh,
                                  const void* queries_dev, int64_t q,
                                  void* points_out_dev,
                                  uint32_t* primitive_ids_out_dev,
                                  void* primitive_uvs_out_dev,
                                  void* primitive_normals_out_dev,
                                  void* distance_out_dev, int sort_queries,
                                  unsigned long long* visits_out,
                                  o3dmi_stream_t stream) {
    O3DMI_REQUIRE(bvh, "null argument");
    const int st = CheckQueries(queries_dev, q, O3DMI_F32);
    if (st) return st;
    if (q == 0) return O3DMI_OK;
    return RunQuery(bvh, queries_dev, q,
                    Outputs(points_out_dev, primitive_ids_out_dev,
                            primitive_uvs_out_dev, primitive_normals_out_dev,
                            distance_out_dev),
                    sort_queries != 0, visits_out, (hipStream_t)stream);
}

int o3dmi_mesh_bvh_closest_points(const o3dmi_mesh_bvh_t* bvh,
                                  const void* queries_dev, int64_t q,
                                  int dtype, void* points_out_dev,
                                  uint32_t* primitive_ids_out_dev,
                                  void* primitive_uvs_out_dev,
                                  void* primitive_normals_out_dev,
                                  void* distance_out_dev,
                                  o3dmi_stream_t stream) {
    O3DMI_REQUIRE(bvh, "null argument");
    const int st = CheckQueries(queries_dev, q, dtype);
    if (st) return st;
    if (q == 0) return O3DMI_OK;
    return RunQuery(bvh, queries_dev, q,
                    Outputs(points_out_dev, primitive_ids_out_dev,
                            primitive_uvs_out_dev, primitive_normals_out_dev,
                            distance_out_dev),
                    kSortQueries, nullptr, (hipStream_t)stream);
}

int o3dmi_trianglemesh_closest_points(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* queries_dev, int64_t q, void* points_out_dev,
        uint32_t* primitive_ids_out_dev, void* primitive_uvs_out_dev,
        void* primitive_normals_out_dev, void* distance_out_dev,
        o3dmi_stream_t stream) {
    int st = CheckSceneMesh(positions_dev, v, dtype, triangles_dev, m,
                            index_dtype);
    if (!st) st = CheckQueries(queries_dev, q, dtype);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    BvhPtr bvh;
    if ((st = CreateBvh(positions_dev, v, triangles_dev, m, index_dtype, &bvh,
                        s)))
        return st;
    if (q == 0) return O3DMI_OK;
    return RunQuery(bvh.get(), queries_dev, q,
                    Outputs(points_out_dev, primitive_ids_out_dev,
                            primitive_uvs_out_dev, primitive_normals_out_dev,
                            distance_out_dev),
                    kSortQueries, nullptr, s);
}

int o3dmi_trianglemesh_compute_distance(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* queries_dev, int64_t q, void* distance_out_dev,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(q <= 0 || distance_out_dev, "null argument");
    return o3dmi_trianglemesh_closest_points(
            positions_dev, v, dtype, triangles_dev, m, index_dtype,
            queries_dev, q, nullptr, nullptr, nullptr, nullptr,
            distance_out_dev, stream);
}

int o3dmi_trianglemesh_compute_metrics(
        const void* positions1_dev, int64_t v1, const void* triangles1_dev,
        int64_t m1, int index_dtype1, const void* positions2_dev, int64_t v2,
        const void* triangles2_dev, int64_t m2, int index_dtype2, int dtype,
        const int32_t* metrics, int n_metrics, const float* fscore_radius,
        int n_radii, int64_t n_sampled_points, uint64_t seed,
        float* values_out, int64_t values_capacity,
        o3dmi_pointcloud_metrics_raw_t* raw_out, o3dmi_stream_t stream) {
    int st = CheckSceneMesh(positions1_dev, v1, dtype, triangles1_dev, m1,
                            index_dtype1);
    if (!st)
        st = CheckSceneMesh(positions2_dev, v2, dtype, triangles2_dev, m2,
                            index_dtype2);
    if (st) return st;
    O3DMI_REQUIRE(v1 > 0 && v2 > 0,
                  "One or both input triangle meshes are empty!");
    O3DMI_REQUIRE(n_sampled_points > 0 && n_sampled_points < (1ll << 31) - 1,
                  "n_sampled_points out of range");
    O3DMI_REQUIRE(n_radii >= 0 && (n_radii == 0 || fscore_radius),
                  "null argument");
    // the list, the capacity and the pointers, before anything runs: the
    // final arithmetic on zeros into a scratch array
    const int64_t n = n_sampled_points;
    {
        const double zero[2] = {0, 0};
        std::vector<int64_t> no_counts((size_t)(2 * n_radii) + 1, 0);
        O3DMI_REQUIRE(values_capacity >= 0, "values_capacity < 0");
        O3DMI_REQUIRE(values_capacity == 0 || values_out, "null argument");
        std::vector<float> trial((size_t)values_capacity + 1);
        st = o3dmi_metrics_from_sums(n, n, zero, zero, no_counts.data(),
                                     n_radii, metrics, n_metrics, trial.data(),
                                     values_capacity);
        if (st) return st;
    }
    hipStream_t s = (hipStream_t)stream;
    Direction dir[2];
    {
        PoolScratch pool(s);
        float *samples1 = nullptr, *samples2 = nullptr;
        if ((st = pool.Alloc(&samples1, sizeof(float) * 3 * (size_t)n)))
            return st;
        if ((st = pool.Alloc(&samples2, sizeof(float) * 3 * (size_t)n)))
            return st;
        MeshSampleIO io = {};
        io.points_out = samples1;
        if ((st = SampleMeshChecked(positions1_dev, v1, O3DMI_F32,
                                    triangles1_dev, m1, index_dtype1, n, seed,
                                    io, s)))
            return st;
        io.points_out = samples2;
        if ((st = SampleMeshChecked(positions2_dev, v2, O3DMI_F32,
                                    triangles2_dev, m2, index_dtype2, n,
                                    seed + 1, io, s)))
            return st;
        BvhPtr bvh1, bvh2;
        if ((st = CreateBvh(positions1_dev, v1, triangles1_dev, m1,
                            index_dtype1, &bvh1, s)))
            return st;
        if ((st = CreateBvh(positions2_dev, v2, triangles2_dev, m2,
                            index_dtype2, &bvh2, s)))
            return st;
        // distance12: the samples of mesh 1 against mesh 2
        if ((st = RunDirection(bvh2.get(), samples1, n, fscore_radius, n_radii,
                               &dir[0], s)))
            return st;
        if ((st = RunDirection(bvh1.get(), samples2, n, fscore_radius, n_radii,
                               &dir[1], s)))
            return st;
    }
    const double sum[2] = {dir[0].sum, dir[1].sum};
    const double max[2] = {dir[0].max, dir[1].max};
    std::vector<int64_t> counts((size_t)(2 * n_radii) + 1);
    for (int r = 0; r < n_radii; ++r) {
        counts[(size_t)r] = dir[0].counts[(size_t)r];
        counts[(size_t)(n_radii + r)] = dir[1].counts[(size_t)r];
    }
    st = o3dmi_metrics_from_sums(n, n, sum, max, counts.data(), n_radii,
                                 metrics, n_metrics, values_out,
                                 values_capacity);
    if (st) return st;
    if (raw_out) {
        for (int d = 0; d < 2; ++d) {
            raw_out->sum[d] = sum[d];
            raw_out->max[d] = max[d];
            raw_out->second_pass_queries[d] = 0;
        }
        if (raw_out->counts)
            std::copy(counts.begin(), counts.begin() + 2 * n_radii,
                      raw_out->counts);
    }
    return O3DMI_OK;
}

}  // extern "C"
