// Host drivers of the TriangleMesh operators: the elementwise kernels of
// t/geometry/kernel/TriangleMesh.h, ComputeVertexNormals, and the host loops
// of t/geometry/TriangleMesh.cpp (SelectFacesByMask:1221, SelectByIndex:1292,
// RemoveUnreferencedVertices:1399, GetNonManifoldEdges:1826) and of legacy
// ClusterConnectedTriangles (geometry/TriangleMesh.cpp:1459) on the device.
// Arguments are checked before anything is allocated, the triangle indices on
// the device before anything is written; the kernels are in trianglemesh.hip.
#include <algorithm>

#include "../scan.h"
#include "../sort.h"
#include "o3d_mi355x_host.h"
#include "trianglemesh_call.h"

using namespace o3dmi;

namespace {

// The arguments of a call on positions and triangles.
int CheckMesh(const void* positions_dev, int64_t v, int dtype,
              const void* triangles_dev, int64_t m, int index_dtype) {
    int st = CheckFloat(dtype);
    if (!st) st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(m == 0 || (positions_dev && triangles_dev), "null argument");
    return O3DMI_OK;
}

// ComputeVertexNormalsCPU on checked triangles (m, v >= 1).
int VertexNormalsOf(PoolScratch& pool, const int32_t* tri, int64_t m,
                    int64_t v, const void* tn_dev, int dtype, void* out_dev) {
    hipStream_t s = pool.s;
    CornerTable tb;
    int32_t* long_list = nullptr;
    void* scratch = nullptr;
    int st = AllocCornerTable(pool, m, v, &tb);
    if (!st) st = pool.Alloc(&scratch, IncidenceScratchBytes(m, v));
    if (!st) st = AllocLongList(pool, v, &long_list);
    if (st) return st;
    if ((st = BuildCornerTableAsync(tri, m, v, tb, scratch, s))) return st;
    return VertexNormalSumAsync(tb, v, tn_dev, dtype, out_dev, long_list, s);
}

// The chain the selections share. vflags {v} / tflags {m} (NULL: every
// triangle kept) hold 0 / 1; v >= 1.
int SelectChain(PoolScratch& pool, Words* w, const int32_t* tri, int64_t m,
                int index_dtype, int64_t v, const int32_t* vflags,
                const int32_t* tflags, uint8_t* vertex_mask_out_dev,
                void* triangles_out_dev, int64_t* n_triangles_out,
                int64_t* n_vertices_out) {
    hipStream_t s = pool.s;
    int64_t* vnew = nullptr;
    int64_t* tpos = nullptr;
    void* scratch = nullptr;
    int st = pool.Alloc(&vnew, sizeof(int64_t) * (size_t)v);
    if (!st && tflags && m > 0)
        st = pool.Alloc(&tpos, sizeof(int64_t) * (size_t)m);
    if (!st) st = pool.Alloc(&scratch, ScanScratchBytes(std::max(v, m)));
    if (st) return st;
    if ((st = PrefixSumAsync(vflags, v, false, vnew, (int64_t*)&w->count,
                             scratch, s)))
        return st;
    if (tpos && (st = PrefixSumAsync(tflags, m, false, tpos,
                                     (int64_t*)&w->total, scratch, s)))
        return st;
    if (m > 0 && (st = RemapTrianglesAsync(tri, m, tflags, tpos, vnew,
                                           index_dtype, triangles_out_dev, s)))
        return st;
    if ((st = FlagsToMaskAsync(vflags, v, vertex_mask_out_dev, s))) return st;
    Words host;
    if ((st = Download(w, &host, sizeof(host), s))) return st;
    *n_vertices_out = (int64_t)host.count;
    *n_triangles_out = tflags ? (int64_t)host.total : m;
    return O3DMI_OK;
}

int SelectFaces(const void* triangles_dev, int64_t m, int index_dtype,
                int64_t v, const uint8_t* tri_mask_dev, bool all_faces,
                uint8_t* vertex_mask_out_dev, void* triangles_out_dev,
                int64_t* n_triangles_out, int64_t* n_vertices_out,
                hipStream_t s) {
    int st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(n_triangles_out && n_vertices_out, "null argument");
    O3DMI_REQUIRE(v == 0 || vertex_mask_out_dev, "null argument");
    O3DMI_REQUIRE(m == 0 || (triangles_dev && triangles_out_dev &&
                             (all_faces || tri_mask_dev)),
                  "null argument");
    if (m == 0) {  // no triangle names a vertex
        if (v > 0) {
            O3DMI_HIP_CHECK(
                    hipMemsetAsync(vertex_mask_out_dev, 0, (size_t)v, s));
            O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        }
        *n_triangles_out = *n_vertices_out = 0;
        return O3DMI_OK;
    }
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    int32_t* vflags = nullptr;
    int32_t* tflags = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    if ((st = pool.Alloc(&vflags, sizeof(int32_t) * (size_t)v))) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(vflags, 0, sizeof(int32_t) * (size_t)v, s));
    if (!all_faces) {
        if ((st = pool.Alloc(&tflags, sizeof(int32_t) * (size_t)m))) return st;
        if ((st = MaskToFlagsAsync(tri_mask_dev, m, tflags, s))) return st;
    }
    if ((st = MarkTriangleVerticesAsync(tri, m, tflags, vflags, s))) return st;
    return SelectChain(pool, w, tri, m, index_dtype, v, vflags, tflags,
                       vertex_mask_out_dev, triangles_out_dev, n_triangles_out,
                       n_vertices_out);
}

}  // namespace

namespace o3dmi {

int SampleMeshChecked(const void* positions_dev, int64_t v, int dtype,
                      const void* triangles_dev, int64_t m, int index_dtype,
                      int64_t n, uint64_t seed, MeshSampleIO io,
                      hipStream_t s) {
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    void* areas = nullptr;
    double* prefix = nullptr;
    int st = AllocWords(pool, &w);
    if (st) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    if ((st = pool.Alloc(&areas, ElemSize(dtype) * (size_t)m))) return st;
    if ((st = pool.Alloc(&prefix, sizeof(double) * MeshPrefixDoubles(m))))
        return st;
    if ((st = TriangleAreasAsync(positions_dev, dtype, tri, m, areas, s)))
        return st;
    MeshPrefixTree tree;
    if ((st = MeshPrefixTreeAsync(areas, m, dtype, prefix, &tree, &w->bad, s)))
        return st;
    int bad = 0;
    double total = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&bad, &w->bad, sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    if ((st = Download(
                 tree.prefix[tree.levels - 1] + (tree.size[tree.levels - 1] - 1),
                 &total, sizeof(total), s)))
        return st;
    O3DMI_REQUIRE(!bad, "sample points: a triangle area is not finite");
    O3DMI_REQUIRE(total - total == 0 && total > 0,
                  "sample points: the surface area is not finite and > 0");
    io.positions = positions_dev;
    io.tri = tri;
    if ((st = MeshSamplePointsAsync(tree, areas, dtype, io, n, seed, s)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

}  // namespace o3dmi

extern "C" {

int o3dmi_mesh_sample_draw(uint64_t seed, int64_t j, double* u_out,
                           float* r1_out, float* r2_out) {
    O3DMI_REQUIRE(j >= 0, "j < 0");
    O3DMI_REQUIRE(u_out && r1_out && r2_out, "null argument");
    const MeshSampleDraw d = DrawMeshSample(seed, (uint64_t)j);
    *u_out = d.u;
    *r1_out = d.r1;
    *r2_out = d.r2;
    return O3DMI_OK;
}

int o3dmi_trianglemesh_sample_points_uniformly(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        int64_t number_of_points, uint64_t seed,
        const void* vertex_normals_dev, const void* triangle_normals_dev,
        const void* vertex_colors_dev, int color_dtype, void* points_out_dev,
        void* normals_out_dev, float* colors_out_dev,
        int32_t* triangles_out_dev, o3dmi_stream_t stream) {
    int st = CheckFloat(dtype);
    if (!st) st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(number_of_points > 0, "number_of_points <= 0");
    O3DMI_REQUIRE(number_of_points < (1ll << 31),
                  "number_of_points out of range (< 2^31)");
    O3DMI_REQUIRE(m > 0, "Input mesh has no triangles. Cannot sample points.");
    O3DMI_REQUIRE(v > 0, "Input mesh is empty. Cannot sample points.");
    O3DMI_REQUIRE(positions_dev && triangles_dev && points_out_dev,
                  "null argument");
    O3DMI_REQUIRE(!normals_out_dev || vertex_normals_dev ||
                          triangle_normals_dev,
                  "null argument: normals wanted, none given");
    O3DMI_REQUIRE(!colors_out_dev || vertex_colors_dev,
                  "null argument: colours wanted, none given");
    O3DMI_REQUIRE(!colors_out_dev || color_dtype == O3DMI_F32 ||
                          color_dtype == O3DMI_U8 || color_dtype == O3DMI_U16,
                  "vertex colours must be Float32, UInt8 or UInt16");
    MeshSampleIO io = {};
    io.vertex_normals = vertex_normals_dev;
    io.triangle_normals = triangle_normals_dev;
    io.vertex_colors = vertex_colors_dev;
    io.color_dtype = color_dtype;
    io.points_out = points_out_dev;
    io.normals_out = normals_out_dev;
    io.colors_out = colors_out_dev;
    io.triangles_out = triangles_out_dev;
    return SampleMeshChecked(positions_dev, v, dtype, triangles_dev, m,
                             index_dtype, number_of_points, seed, io,
                             (hipStream_t)stream);
}

int o3dmi_trianglemesh_compute_triangle_normals(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        void* normals_out_dev, o3dmi_stream_t stream) {
    int st = CheckMesh(positions_dev, v, dtype, triangles_dev, m, index_dtype);
    if (st) return st;
    if (m == 0) return O3DMI_OK;
    O3DMI_REQUIRE(normals_out_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    if ((st = TriangleNormalsAsync(positions_dev, dtype, tri, m,
                                   normals_out_dev, s)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_trianglemesh_compute_triangle_areas(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        void* areas_out_dev, o3dmi_stream_t stream) {
    int st = CheckMesh(positions_dev, v, dtype, triangles_dev, m, index_dtype);
    if (st) return st;
    if (m == 0) return O3DMI_OK;
    O3DMI_REQUIRE(areas_out_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    if ((st = TriangleAreasAsync(positions_dev, dtype, tri, m, areas_out_dev,
                                 s)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_trianglemesh_surface_area(const void* positions_dev, int64_t v,
                                    int dtype, const void* triangles_dev,
                                    int64_t m, int index_dtype,
                                    double* area_out, o3dmi_stream_t stream) {
    int st = CheckMesh(positions_dev, v, dtype, triangles_dev, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(area_out, "null argument");
    if (m == 0) {
        *area_out = 0.0;
        return O3DMI_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    void* areas = nullptr;
    double* sums = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    if ((st = pool.Alloc(&areas, ElemSize(dtype) * (size_t)m))) return st;
    if ((st = pool.Alloc(&sums, sizeof(double) * RunSumScratchDoubles(m))))
        return st;
    if ((st = TriangleAreasAsync(positions_dev, dtype, tri, m, areas, s)))
        return st;
    const double* total = nullptr;
    if ((st = RunSumTreeAsync(areas, m, dtype, sums, &total, s))) return st;
    double area = 0;
    if ((st = Download(total, &area, sizeof(area), s))) return st;
    *area_out = area;
    return O3DMI_OK;
}

int o3dmi_trianglemesh_normalize_normals(void* normals_dev, int64_t n,
                                         int dtype, o3dmi_stream_t stream) {
    int st = CheckFloat(dtype);
    if (st) return st;
    O3DMI_REQUIRE(n >= 0 && n < (1ll << 31), "n out of range (< 2^31)");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(normals_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if ((st = NormalizeMeshNormalsAsync(normals_dev, n, dtype, s))) return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_trianglemesh_compute_vertex_normals(
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* triangle_normals_dev, int dtype, int64_t v,
        void* vertex_normals_out_dev, o3dmi_stream_t stream) {
    int st = CheckFloat(dtype);
    if (!st) st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(m == 0 || (triangles_dev && triangle_normals_dev),
                  "null argument");
    O3DMI_REQUIRE(v == 0 || vertex_normals_out_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    if (m > 0) {
        Words* w = nullptr;
        const int32_t* tri = nullptr;
        if ((st = AllocWords(pool, &w))) return st;
        if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v,
                                &tri)))
            return st;
        if ((st = VertexNormalsOf(pool, tri, m, v, triangle_normals_dev, dtype,
                                  vertex_normals_out_dev)))
            return st;
    } else if (v > 0) {
        O3DMI_HIP_CHECK(hipMemsetAsync(vertex_normals_out_dev, 0,
                                       3 * ElemSize(dtype) * (size_t)v, s));
    }
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_trianglemesh_vertex_normals(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        void* triangle_normals_out_dev, void* vertex_normals_out_dev,
        int normalized, o3dmi_stream_t stream) {
    int st = CheckMesh(positions_dev, v, dtype, triangles_dev, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(v == 0 || vertex_normals_out_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    if (m > 0) {
        Words* w = nullptr;
        const int32_t* tri = nullptr;
        void* tn = triangle_normals_out_dev;
        if ((st = AllocWords(pool, &w))) return st;
        if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v,
                                &tri)))
            return st;
        if (!tn && (st = pool.Alloc(&tn, 3 * ElemSize(dtype) * (size_t)m)))
            return st;
        if ((st = TriangleNormalsAsync(positions_dev, dtype, tri, m, tn, s)))
            return st;
        if ((st = VertexNormalsOf(pool, tri, m, v, tn, dtype,
                                  vertex_normals_out_dev)))
            return st;
        if (normalized && (st = NormalizeMeshNormalsAsync(
                                   vertex_normals_out_dev, v, dtype, s)))
            return st;
    } else if (v > 0) {
        // zero rows stay zero under the normalisation (norm > 0 fails)
        O3DMI_HIP_CHECK(hipMemsetAsync(vertex_normals_out_dev, 0,
                                       3 * ElemSize(dtype) * (size_t)v, s));
    }
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_trianglemesh_get_non_manifold_edges(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        int allow_boundary_edges, void* edges_out_dev, int64_t capacity,
        int64_t* n_edges_out, o3dmi_stream_t stream) {
    int st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(n_edges_out, "null argument");
    O3DMI_REQUIRE(m == 0 || triangles_dev, "null argument");
    O3DMI_REQUIRE(capacity <= 0 || edges_out_dev, "null argument");
    if (m == 0) {
        *n_edges_out = 0;
        return O3DMI_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    EdgeTable tb;
    void* scratch = nullptr;
    int32_t* flags = nullptr;
    int64_t* pos = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    if ((st = AllocEdgeTable(pool, 3 * m, &tb))) return st;
    if ((st = pool.Alloc(&scratch, IncidenceScratchBytes(m, v)))) return st;
    if ((st = pool.Alloc(&flags, sizeof(int32_t) * 3 * (size_t)m))) return st;
    if ((st = pool.Alloc(&pos, sizeof(int64_t) * 3 * (size_t)m))) return st;
    if ((st = BuildEdgeTableAsync(tri, m, v, tb, scratch, s))) return st;
    if ((st = NonManifoldFlagsAsync(tb, 3 * m, allow_boundary_edges != 0,
                                    flags, s)))
        return st;
    if ((st = PrefixSumAsync(flags, 3 * m, false, pos, (int64_t*)&w->count,
                             scratch, s)))
        return st;
    int64_t n_edges = 0;
    if ((st = DownloadCount(w, &n_edges, s))) return st;
    *n_edges_out = n_edges;
    if (capacity < 0 || n_edges == 0) return O3DMI_OK;
    if (capacity < n_edges)
        return CapacityError("non-manifold edges: capacity too small");
    if ((st = EmitEdgesAsync(tb, 3 * m, flags, pos, index_dtype,
                             edges_out_dev, s)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_trianglemesh_cluster_connected_triangles(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        int32_t* labels_out_dev, int64_t* n_clusters_out,
        int64_t* cluster_n_triangles_out_dev, double* cluster_area_out_dev,
        int64_t capacity, o3dmi_stream_t stream) {
    int st = CheckSizes(v, m, index_dtype);
    if (!st && cluster_area_out_dev) st = CheckFloat(dtype);
    if (st) return st;
    O3DMI_REQUIRE(n_clusters_out, "null argument");
    O3DMI_REQUIRE(m == 0 || triangles_dev, "null argument");
    O3DMI_REQUIRE(m == 0 || capacity < 0 || labels_out_dev, "null argument");
    O3DMI_REQUIRE(m == 0 || !cluster_area_out_dev || positions_dev,
                  "null argument");
    if (m == 0) {
        *n_clusters_out = 0;
        return O3DMI_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    EdgeTable tb;
    void* scratch = nullptr;
    int *parent = nullptr, *root = nullptr;
    int32_t* is_root = nullptr;
    int64_t* rank = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    if ((st = AllocEdgeTable(pool, 3 * m, &tb))) return st;
    if ((st = pool.Alloc(&scratch, IncidenceScratchBytes(m, v)))) return st;
    if ((st = pool.Alloc(&parent, sizeof(int) * (size_t)m))) return st;
    if ((st = pool.Alloc(&root, sizeof(int) * (size_t)m))) return st;
    if ((st = pool.Alloc(&is_root, sizeof(int32_t) * (size_t)m))) return st;
    if ((st = pool.Alloc(&rank, sizeof(int64_t) * (size_t)m))) return st;
    if ((st = BuildEdgeTableAsync(tri, m, v, tb, scratch, s))) return st;
    if ((st = ClusterRootsAsync(tb, m, parent, root, is_root, s))) return st;
    if ((st = PrefixSumAsync(is_root, m, false, rank, (int64_t*)&w->count,
                             scratch, s)))
        return st;
    int64_t c = 0;
    if ((st = DownloadCount(w, &c, s))) return st;
    *n_clusters_out = c;
    if (capacity < 0) return O3DMI_OK;
    if (capacity < c)
        return CapacityError("cluster_connected_triangles: capacity too small");
    int32_t* counts = nullptr;
    if ((st = pool.Alloc(&counts, sizeof(int32_t) * (size_t)c))) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)c, s));
    if ((st = ClusterLabelsAsync(root, rank, m, labels_out_dev, counts, s)))
        return st;
    if (cluster_n_triangles_out_dev &&
        (st = WidenCountsAsync(counts, c, cluster_n_triangles_out_dev, s)))
        return st;
    if (cluster_area_out_dev) {
        // the edge table is done with: its arrays carry the (label, triangle)
        // pairs
        uint32_t *keys = tb.lo, *members = tb.hi;
        double *area = nullptr, *run_sums = nullptr;
        int64_t *start = nullptr, *run_start = nullptr;
        int32_t* runs = nullptr;
        const int64_t max_runs = m / kMeshRun + c;
        if ((st = pool.Alloc(&area, sizeof(double) * (size_t)m))) return st;
        if ((st = pool.Alloc(&run_sums, sizeof(double) * (size_t)max_runs)))
            return st;
        if ((st = pool.Alloc(&start, sizeof(int64_t) * (size_t)c))) return st;
        if ((st = pool.Alloc(&run_start, sizeof(int64_t) * (size_t)c)))
            return st;
        if ((st = pool.Alloc(&runs, sizeof(int32_t) * (size_t)c))) return st;
        if ((st = TriangleAreasF64Async(positions_dev, dtype, tri, m, area, s)))
            return st;
        if ((st = LabelPairsAsync(labels_out_dev, m, keys, members, s)))
            return st;
        if ((st = SortPairsAsync(keys, members, m, BitsFor(c), scratch, s)))
            return st;
        if ((st = PrefixSumAsync(counts, c, false, start, nullptr, scratch, s)))
            return st;
        if ((st = ClusterRunCountsAsync(counts, c, runs, s))) return st;
        if ((st = PrefixSumAsync(runs, c, false, run_start, nullptr, scratch,
                                 s)))
            return st;
        if ((st = ClusterAreaSumsAsync(area, members, counts, start, run_start,
                                       c, max_runs, run_sums,
                                       cluster_area_out_dev, s)))
            return st;
    }
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_trianglemesh_select_faces_by_mask(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        const uint8_t* tri_mask_dev, uint8_t* vertex_mask_out_dev,
        void* triangles_out_dev, int64_t* n_triangles_out,
        int64_t* n_vertices_out, o3dmi_stream_t stream) {
    return SelectFaces(triangles_dev, m, index_dtype, v, tri_mask_dev, false,
                       vertex_mask_out_dev, triangles_out_dev, n_triangles_out,
                       n_vertices_out, (hipStream_t)stream);
}

int o3dmi_trianglemesh_remove_unreferenced_vertices(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        uint8_t* vertex_mask_out_dev, void* triangles_out_dev,
        int64_t* n_vertices_out, o3dmi_stream_t stream) {
    int64_t n_triangles = 0;
    O3DMI_REQUIRE(n_vertices_out, "null argument");
    return SelectFaces(triangles_dev, m, index_dtype, v, nullptr, true,
                       vertex_mask_out_dev, triangles_out_dev, &n_triangles,
                       n_vertices_out, (hipStream_t)stream);
}

int o3dmi_trianglemesh_select_by_index(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        const int64_t* indices_dev, int64_t k, uint8_t* vertex_mask_out_dev,
        uint8_t* tri_mask_out_dev, void* triangles_out_dev,
        int64_t* n_triangles_out, int64_t* n_vertices_out,
        int64_t* n_ignored_out, o3dmi_stream_t stream) {
    int st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(k >= 0, "k < 0");
    O3DMI_REQUIRE(n_triangles_out && n_vertices_out && n_ignored_out,
                  "null argument");
    O3DMI_REQUIRE(k == 0 || indices_dev, "null argument");
    O3DMI_REQUIRE(v == 0 || vertex_mask_out_dev, "null argument");
    O3DMI_REQUIRE(m == 0 || (triangles_dev && tri_mask_out_dev &&
                             triangles_out_dev),
                  "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (v == 0 && m == 0) {  // every index is out of range
        *n_triangles_out = *n_vertices_out = 0;
        *n_ignored_out = k;
        return O3DMI_OK;
    }
    PoolScratch pool(s);
    Words* w = nullptr;
    unsigned long long* ignored = nullptr;
    const int32_t* tri = nullptr;
    int32_t* vflags = nullptr;
    int32_t* tflags = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = pool.Alloc(&ignored, 256))) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(ignored, 0, sizeof(*ignored), s));
    if (m > 0 && (st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v,
                                     &tri)))
        return st;
    // v >= 1 from here: a triangle list with v == 0 has failed its check
    if ((st = pool.Alloc(&vflags, sizeof(int32_t) * (size_t)v))) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(vflags, 0, sizeof(int32_t) * (size_t)v, s));
    if (k > 0 && (st = MarkIndexedVerticesAsync(indices_dev, k, v, vflags,
                                                ignored, s)))
        return st;
    if (m > 0) {
        if ((st = pool.Alloc(&tflags, sizeof(int32_t) * (size_t)m))) return st;
        if ((st = TrianglesOfVerticesAsync(tri, m, vflags, tflags, s)))
            return st;
        if ((st = FlagsToMaskAsync(tflags, m, tri_mask_out_dev, s))) return st;
    }
    unsigned long long n_ignored = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&n_ignored, ignored, sizeof(n_ignored),
                                   hipMemcpyDeviceToHost, s));
    st = SelectChain(pool, w, tri, m, index_dtype, v, vflags, tflags,
                     vertex_mask_out_dev, triangles_out_dev, n_triangles_out,
                     n_vertices_out);
    if (st) return st;
    *n_ignored_out = (int64_t)n_ignored;
    return O3DMI_OK;
}

}  // extern "C"
