// Host drivers of the closest-point queries on a triangle mesh
// (RaycastingScene::ComputeClosestPoints / ComputeDistance for one triangle
// geometry, t/geometry/RaycastingScene.cpp:1464-1517), of
// TriangleMesh::ComputeMetrics (t/geometry/TriangleMesh.cpp:1939-1967) and
// of the ray queries on the same handle (RaycastingScene.cpp:1325-1462,
// 1520-1674).
// Arguments are checked before anything is allocated, the triangle indices
// and the coordinates on the device before anything is written; the kernels
// are in mesh_bvh.hip.
#include <algorithm>
#include <cmath>
#include <memory>
#include <random>
#include <vector>

#include "../mesh_bvh.h"
#include "../pointcloud_metrics.h"
#include "../scan.h"
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
        if ((st = Download(scene, bvh->scene, 6 * sizeof(float), s)))
            return st;
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
    if ((st = Download(total, &dir->sum, sizeof(double), s))) return st;
    std::memcpy(&dir->max, &host[0].max_bits, sizeof(double));
    dir->counts.resize((size_t)n_radii);
    for (int r = 0; r < n_radii; ++r)
        dir->counts[(size_t)r] = (int64_t)host[(size_t)(r / kMetricsRadiusGroup)]
                                         .counts[r % kMetricsRadiusGroup];
    return O3DMI_OK;
}

// ---- ray queries ----------------------------------------------------------------
int CheckRays(const void* rays_dev, int64_t q, int dtype) {
    // 2 q rows of three go through the finiteness gate
    O3DMI_REQUIRE(q >= 0 && q < (1ll << 30), "q out of range (< 2^30 rays)");
    if (dtype == O3DMI_F64)
        return Unsupported("ray queries: Float32 only (upstream's scene)");
    O3DMI_REQUIRE(dtype == O3DMI_F32, "rays must be Float32");
    O3DMI_REQUIRE(q == 0 || rays_dev, "null argument");
    return O3DMI_OK;
}

int OverflowStatus(int overflow) {
    if (!overflow) return O3DMI_OK;
    SetLastError("ray query: traversal stack overflow");
    return O3DMI_ERR_INTERNAL;
}

// Checked rays (q > 0) against a complete handle. Waits.
int RunRayQuery(const o3dmi_mesh_bvh* bvh, RayQueryKind kind,
                const void* rays_dev, int64_t q, float tnear, float tfar,
                const RayQueryOut& out, bool sort_rays,
                unsigned long long* visits_out, hipStream_t s) {
    O3DMI_REQUIRE(tnear == tnear && tfar == tfar, "tnear / tfar is NaN");
    PoolScratch pool(s);
    Words* w = nullptr;
    unsigned long long* visits = nullptr;
    void* scratch = nullptr;
    int st = AllocWords(pool, &w);
    if (st) return st;
    if ((st = RequireFinite(rays_dev, 2 * q, O3DMI_F32, w, s))) return st;
    if (visits_out) {
        if ((st = pool.Alloc(&visits, 256))) return st;
        O3DMI_HIP_CHECK(hipMemsetAsync(visits, 0, 16, s));
    }
    if (sort_rays && (st = pool.Alloc(&scratch, MeshBvhQueryScratchBytes(q))))
        return st;
    // w->bad is still zero: RequireFinite passed
    if ((st = MeshBvhRayQueryAsync(ViewOf(bvh), kind, (const float*)rays_dev,
                                   q, tnear, tfar, out, sort_rays, scratch,
                                   &w->bad, visits, s)))
        return st;
    int overflow = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&overflow, &w->bad, sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    if (visits_out)
        O3DMI_HIP_CHECK(hipMemcpyAsync(visits_out, visits, 16,
                                       hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return OverflowStatus(overflow);
}

RayQueryOut CastOutputs(void* t_hit, uint32_t* geometry_ids,
                        uint32_t* primitive_ids, void* uvs, void* normals) {
    RayQueryOut out = {};
    out.t_hit = (float*)t_hit;
    out.geometry_ids = geometry_ids;
    out.primitive_ids = primitive_ids;
    out.uvs = (float*)uvs;
    out.normals = (float*)normals;
    return out;
}

// The count pass, the scan and the write pass of ListIntersections. Waits.
int RunRayList(const o3dmi_mesh_bvh* bvh, const void* rays_dev, int64_t q,
               int64_t* splits_out_dev, int64_t capacity, int64_t* total_out,
               const RayListOut& out, hipStream_t s) {
    PoolScratch pool(s);
    Words* w = nullptr;
    int32_t* counts = nullptr;
    void* scan_scratch = nullptr;
    int64_t* splits = splits_out_dev;
    int st = AllocWords(pool, &w);
    if (st) return st;
    if ((st = RequireFinite(rays_dev, 2 * q, O3DMI_F32, w, s))) return st;
    if ((st = pool.Alloc(&counts, sizeof(int32_t) * (size_t)q))) return st;
    if ((st = pool.Alloc(&scan_scratch, ScanScratchBytes(q)))) return st;
    if (!splits &&
        (st = pool.Alloc(&splits, sizeof(int64_t) * (size_t)(q + 1))))
        return st;
    const MeshBvhView view = ViewOf(bvh);
    RayQueryOut count_out = {};
    count_out.counts = counts;
    if ((st = MeshBvhRayQueryAsync(view, kRayCount, (const float*)rays_dev, q,
                                   0.0f, INFINITY, count_out, false, nullptr,
                                   &w->bad, nullptr, s)))
        return st;
    if ((st = PrefixSumAsync(counts, q, false, splits, (int64_t*)&w->total,
                             scan_scratch, s)))
        return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(splits + q, &w->total, sizeof(int64_t),
                                   hipMemcpyDeviceToDevice, s));
    Words host = {};
    if ((st = Download(w, &host, sizeof(host), s))) return st;
    if ((st = OverflowStatus(host.bad))) return st;
    const int64_t total = (int64_t)host.total;
    *total_out = total;
    if (total > 0x7FFFFFFFll)
        return Unsupported("list intersections: more than 2^31 - 1 entries");
    if (capacity < 0 || total == 0) return O3DMI_OK;
    if (capacity < total)
        return CapacityError("list intersections: capacity too small");
    if ((st = MeshBvhRayListAsync(view, (const float*)rays_dev, q, splits, out,
                                  &w->bad, s)))
        return st;
    int overflow = 0;
    if ((st = Download(&w->bad, &overflow, sizeof(overflow), s))) return st;
    return OverflowStatus(overflow);
}

int CheckSamples(int nsamples) {
    O3DMI_REQUIRE(nsamples >= 1 && (nsamples % 2) == 1,
                  "nsamples must be odd and >= 1");
    return O3DMI_OK;
}

// VoteInsideOutside's directions: upstream's statements, the 3 x nsamples
// matrix filled in column-major order (Eigen's assignment of a unaryExpr to a
// column-major matrix walks every column from top to bottom).
void VoteDirections(int nsamples, float* out) {
    std::mt19937 gen(42);
    std::uniform_real_distribution<float> dist(-0.001, 0.001);
    for (int j = 0; j < 3 * nsamples; ++j) out[j] = 1 + dist(gen);
}

// Checked points (q > 0): the closest-point distance when distance_out_dev
// is wanted, then the vote that signs it. Waits.
int RunVote(const o3dmi_mesh_bvh* bvh, const void* points_dev, int64_t q,
            int nsamples, float* occupancy_out_dev, float* distance_out_dev,
            hipStream_t s) {
    if (distance_out_dev) {
        // checks the points as well
        MeshQueryOut out = {};
        out.distance = distance_out_dev;
        const int st = RunQuery(bvh, points_dev, q, out, kSortQueries, nullptr,
                                s);
        if (st) return st;
    }
    PoolScratch pool(s);
    Words* w = nullptr;
    float* dirs = nullptr;
    int st = AllocWords(pool, &w);
    if (st) return st;
    if (!distance_out_dev &&
        (st = RequireFinite(points_dev, q, O3DMI_F32, w, s)))
        return st;
    std::vector<float> host_dirs(3 * (size_t)nsamples);
    VoteDirections(nsamples, host_dirs.data());
    if ((st = pool.Alloc(&dirs, sizeof(float) * host_dirs.size()))) return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(dirs, host_dirs.data(),
                                   sizeof(float) * host_dirs.size(),
                                   hipMemcpyHostToDevice, s));
    if ((st = MeshBvhVoteAsync(ViewOf(bvh), (const float*)points_dev, q, dirs,
                               nsamples, occupancy_out_dev, distance_out_dev,
                               &w->bad, s)))
        return st;
    int overflow = 0;
    // host_dirs is pageable: the upload above was staged before it returned
    if ((st = Download(&w->bad, &overflow, sizeof(overflow), s))) return st;
    return OverflowStatus(overflow);
}

// The adjugate of a row-major 3 x 3 over its determinant, in double.
void Inverse3(const double k[9], double out[9]) {
    const double c00 = k[4] * k[8] - k[5] * k[7];
    const double c01 = k[5] * k[6] - k[3] * k[8];
    const double c02 = k[3] * k[7] - k[4] * k[6];
    const double det = (k[0] * c00 + k[1] * c01) + k[2] * c02;
    out[0] = c00 / det;
    out[1] = (k[2] * k[7] - k[1] * k[8]) / det;
    out[2] = (k[1] * k[5] - k[2] * k[4]) / det;
    out[3] = c01 / det;
    out[4] = (k[0] * k[8] - k[2] * k[6]) / det;
    out[5] = (k[2] * k[3] - k[0] * k[5]) / det;
    out[6] = c02 / det;
    out[7] = (k[1] * k[6] - k[0] * k[7]) / det;
    out[8] = (k[0] * k[4] - k[1] * k[3]) / det;
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

// ---- ray queries ----------------------------------------------------------------
int o3dmi_internal_mesh_bvh_ray_query(
        const o3dmi_mesh_bvh* bvh, int kind, const void* rays_dev, int64_t q,
        float tnear, float tfar, void* t_hit_out_dev,
        uint32_t* geometry_ids_out_dev, uint32_t* primitive_ids_out_dev,
        void* primitive_uvs_out_dev, void* primitive_normals_out_dev,
        uint8_t* occluded_out_dev, int32_t* counts_out_dev, int sort_rays,
        unsigned long long* visits_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(bvh, "null argument");
    O3DMI_REQUIRE(kind >= kRayClosest && kind <= kRayCount,
                  "unknown ray query kind");
    const int st = CheckRays(rays_dev, q, O3DMI_F32);
    if (st) return st;
    O3DMI_REQUIRE(tnear == tnear && tfar == tfar, "tnear / tfar is NaN");
    if (q == 0) return O3DMI_OK;
    RayQueryOut out = CastOutputs(t_hit_out_dev, geometry_ids_out_dev,
                                  primitive_ids_out_dev, primitive_uvs_out_dev,
                                  primitive_normals_out_dev);
    out.occluded = occluded_out_dev;
    out.counts = counts_out_dev;
    return RunRayQuery(bvh, (RayQueryKind)kind, rays_dev, q, tnear, tfar, out,
                       sort_rays != 0, visits_out, (hipStream_t)stream);
}

int o3dmi_mesh_bvh_cast_rays(const o3dmi_mesh_bvh_t* bvh, const void* rays_dev,
                             int64_t q, int dtype, void* t_hit_out_dev,
                             uint32_t* geometry_ids_out_dev,
                             uint32_t* primitive_ids_out_dev,
                             void* primitive_uvs_out_dev,
                             void* primitive_normals_out_dev,
                             o3dmi_stream_t stream) {
    O3DMI_REQUIRE(bvh, "null argument");
    const int st = CheckRays(rays_dev, q, dtype);
    if (st) return st;
    if (q == 0) return O3DMI_OK;
    return RunRayQuery(bvh, kRayClosest, rays_dev, q, 0.0f, INFINITY,
                       CastOutputs(t_hit_out_dev, geometry_ids_out_dev,
                                   primitive_ids_out_dev,
                                   primitive_uvs_out_dev,
                                   primitive_normals_out_dev),
                       kSortQueries, nullptr, (hipStream_t)stream);
}

int o3dmi_mesh_bvh_test_occlusions(const o3dmi_mesh_bvh_t* bvh,
                                   const void* rays_dev, int64_t q, int dtype,
                                   float tnear, float tfar,
                                   uint8_t* occluded_out_dev,
                                   o3dmi_stream_t stream) {
    O3DMI_REQUIRE(bvh, "null argument");
    const int st = CheckRays(rays_dev, q, dtype);
    if (st) return st;
    O3DMI_REQUIRE(tnear == tnear && tfar == tfar, "tnear / tfar is NaN");
    O3DMI_REQUIRE(q == 0 || occluded_out_dev, "null argument");
    if (q == 0) return O3DMI_OK;
    RayQueryOut out = {};
    out.occluded = occluded_out_dev;
    return RunRayQuery(bvh, kRayAny, rays_dev, q, tnear, tfar, out,
                       kSortQueries, nullptr, (hipStream_t)stream);
}

int o3dmi_mesh_bvh_count_intersections(const o3dmi_mesh_bvh_t* bvh,
                                       const void* rays_dev, int64_t q,
                                       int dtype, int32_t* counts_out_dev,
                                       o3dmi_stream_t stream) {
    O3DMI_REQUIRE(bvh, "null argument");
    const int st = CheckRays(rays_dev, q, dtype);
    if (st) return st;
    O3DMI_REQUIRE(q == 0 || counts_out_dev, "null argument");
    if (q == 0) return O3DMI_OK;
    RayQueryOut out = {};
    out.counts = counts_out_dev;
    return RunRayQuery(bvh, kRayCount, rays_dev, q, 0.0f, INFINITY, out,
                       kSortQueries, nullptr, (hipStream_t)stream);
}

int o3dmi_mesh_bvh_list_intersections(
        const o3dmi_mesh_bvh_t* bvh, const void* rays_dev, int64_t q,
        int dtype, int64_t* ray_splits_out_dev, int64_t capacity,
        int64_t* total_out, int64_t* ray_ids_out_dev, void* t_hit_out_dev,
        uint32_t* geometry_ids_out_dev, uint32_t* primitive_ids_out_dev,
        void* primitive_uvs_out_dev, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(bvh && total_out, "null argument");
    const int st = CheckRays(rays_dev, q, dtype);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    if (q == 0) {
        *total_out = 0;
        if (ray_splits_out_dev) {
            O3DMI_HIP_CHECK(hipMemsetAsync(ray_splits_out_dev, 0,
                                           sizeof(int64_t), s));
            O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        }
        return O3DMI_OK;
    }
    RayListOut out = {};
    out.ray_ids = ray_ids_out_dev;
    out.t_hit = (float*)t_hit_out_dev;
    out.geometry_ids = geometry_ids_out_dev;
    out.primitive_ids = primitive_ids_out_dev;
    out.uvs = (float*)primitive_uvs_out_dev;
    return RunRayList(bvh, rays_dev, q, ray_splits_out_dev, capacity,
                      total_out, out, s);
}

int o3dmi_mesh_bvh_compute_occupancy(const o3dmi_mesh_bvh_t* bvh,
                                     const void* points_dev, int64_t q,
                                     int dtype, int nsamples,
                                     void* occupancy_out_dev,
                                     o3dmi_stream_t stream) {
    O3DMI_REQUIRE(bvh, "null argument");
    int st = CheckQueries(points_dev, q, dtype);
    if (!st) st = CheckSamples(nsamples);
    if (st) return st;
    O3DMI_REQUIRE(q == 0 || occupancy_out_dev, "null argument");
    if (q == 0) return O3DMI_OK;
    return RunVote(bvh, points_dev, q, nsamples, (float*)occupancy_out_dev,
                   nullptr, (hipStream_t)stream);
}

int o3dmi_mesh_bvh_compute_signed_distance(const o3dmi_mesh_bvh_t* bvh,
                                           const void* points_dev, int64_t q,
                                           int dtype, int nsamples,
                                           void* distance_out_dev,
                                           o3dmi_stream_t stream) {
    O3DMI_REQUIRE(bvh, "null argument");
    int st = CheckQueries(points_dev, q, dtype);
    if (!st) st = CheckSamples(nsamples);
    if (st) return st;
    O3DMI_REQUIRE(q == 0 || distance_out_dev, "null argument");
    if (q == 0) return O3DMI_OK;
    return RunVote(bvh, points_dev, q, nsamples, nullptr,
                   (float*)distance_out_dev, (hipStream_t)stream);
}

int o3dmi_raycast_vote_directions(int nsamples, float* out) {
    const int st = CheckSamples(nsamples);
    if (st) return st;
    O3DMI_REQUIRE(out, "null argument");
    VoteDirections(nsamples, out);
    return O3DMI_OK;
}

int o3dmi_create_rays_pinhole(const double* intrinsic, const double* extrinsic,
                              int width, int height, void* rays_out_dev,
                              o3dmi_stream_t stream) {
    O3DMI_REQUIRE(intrinsic && extrinsic, "null argument");
    O3DMI_REQUIRE(width > 0 && height > 0 &&
                          (int64_t)width * height < (1ll << 30),
                  "width / height out of range");
    O3DMI_REQUIRE(rays_out_dev, "null argument");
    for (int k = 0; k < 9; ++k)
        O3DMI_REQUIRE(std::isfinite(intrinsic[k]), "non-finite intrinsic");
    for (int k = 0; k < 16; ++k)
        O3DMI_REQUIRE(std::isfinite(extrinsic[k]), "non-finite extrinsic");
    double inv_k[9];
    Inverse3(intrinsic, inv_k);
    PinholeFrame frame;
    for (int i = 0; i < 3; ++i) {
        // row i of R^T is column i of R
        const double r0 = extrinsic[i], r1 = extrinsic[4 + i],
                     r2 = extrinsic[8 + i];
        frame.centre[i] = (float)-((r0 * extrinsic[3] + r1 * extrinsic[7]) +
                                   r2 * extrinsic[11]);
        for (int j = 0; j < 3; ++j)
            frame.dir[3 * i + j] = (float)((r0 * inv_k[j] + r1 * inv_k[3 + j]) +
                                           r2 * inv_k[6 + j]);
    }
    for (int k = 0; k < 3; ++k)
        O3DMI_REQUIRE(std::isfinite(frame.centre[k]), "singular camera");
    for (int k = 0; k < 9; ++k)
        O3DMI_REQUIRE(std::isfinite(frame.dir[k]), "singular intrinsic");
    hipStream_t s = (hipStream_t)stream;
    const int st = CreateRaysPinholeAsync(frame, width, height,
                                          (float*)rays_out_dev, s);
    if (st) return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_trianglemesh_cast_rays(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* rays_dev, int64_t q, void* t_hit_out_dev,
        uint32_t* geometry_ids_out_dev, uint32_t* primitive_ids_out_dev,
        void* primitive_uvs_out_dev, void* primitive_normals_out_dev,
        o3dmi_stream_t stream) {
    int st = CheckSceneMesh(positions_dev, v, dtype, triangles_dev, m,
                            index_dtype);
    if (!st) st = CheckRays(rays_dev, q, dtype);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    BvhPtr bvh;
    if ((st = CreateBvh(positions_dev, v, triangles_dev, m, index_dtype, &bvh,
                        s)))
        return st;
    if (q == 0) return O3DMI_OK;
    return RunRayQuery(bvh.get(), kRayClosest, rays_dev, q, 0.0f, INFINITY,
                       CastOutputs(t_hit_out_dev, geometry_ids_out_dev,
                                   primitive_ids_out_dev,
                                   primitive_uvs_out_dev,
                                   primitive_normals_out_dev),
                       kSortQueries, nullptr, s);
}

int o3dmi_trianglemesh_compute_signed_distance(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* points_dev, int64_t q, int nsamples,
        void* distance_out_dev, o3dmi_stream_t stream) {
    int st = CheckSceneMesh(positions_dev, v, dtype, triangles_dev, m,
                            index_dtype);
    if (!st) st = CheckQueries(points_dev, q, dtype);
    if (!st) st = CheckSamples(nsamples);
    if (st) return st;
    O3DMI_REQUIRE(q == 0 || distance_out_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    BvhPtr bvh;
    if ((st = CreateBvh(positions_dev, v, triangles_dev, m, index_dtype, &bvh,
                        s)))
        return st;
    if (q == 0) return O3DMI_OK;
    return RunVote(bvh.get(), points_dev, q, nsamples, nullptr,
                   (float*)distance_out_dev, s);
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
