// Host drivers of the mesh clean-up calls, the CSR adjacency and the vertex
// clustering: legacy RemoveDuplicatedVertices / RemoveDuplicatedTriangles /
// RemoveDegenerateTriangles / ComputeAdjacencyList (geometry/TriangleMesh.cpp:
// 153-165, 680-860) and SimplifyVertexClustering (TriangleMeshSimplification.
// cpp:72-244) as chains of the representative table, the scan, the pair sort
// and the incidence tables. Arguments are checked before anything is
// allocated, the triangle indices on the device before anything is written;
// the kernels are in trianglemesh_clean.hip.
#include <algorithm>
#include <climits>

#include "../pointcloud_sample.h"
#include "../scan.h"
#include "../sort.h"
#include "../trianglemesh_clean.h"
#include "o3d_mi355x_host.h"
#include "trianglemesh_call.h"

using namespace o3dmi;

namespace {

// The representative table of n rows: rep {n}, first {n} and the table.
struct RepBuffers {
    int32_t* table;
    int64_t slots;
    int32_t* rep;
    int32_t* first;
};

int AllocRep(PoolScratch& pool, int64_t n, RepBuffers* r) {
    r->slots = RepTableSlots(n);
    int st = pool.Alloc(&r->table, sizeof(int32_t) * (size_t)r->slots);
    if (!st) st = pool.Alloc(&r->rep, sizeof(int32_t) * (size_t)n);
    if (!st) st = pool.Alloc(&r->first, sizeof(int32_t) * (size_t)n);
    return st;
}

// The triangles with flags != 0, in order and unchanged, their mask and their
// number (one wait).
int KeepTriangles(PoolScratch& pool, Words* w, const int32_t* tri, int64_t m,
                  int index_dtype, const int32_t* flags,
                  uint8_t* tri_mask_out_dev, void* triangles_out_dev,
                  int64_t* n_triangles_out) {
    hipStream_t s = pool.s;
    int64_t* pos = nullptr;
    void* scratch = nullptr;
    int st = pool.Alloc(&pos, sizeof(int64_t) * (size_t)m);
    if (!st) st = pool.Alloc(&scratch, ScanScratchBytes(m));
    if (st) return st;
    if ((st = PrefixSumAsync(flags, m, false, pos, (int64_t*)&w->count, scratch,
                             s)))
        return st;
    if ((st = CompactTrianglesAsync(tri, m, flags, pos, index_dtype,
                                    triangles_out_dev, s)))
        return st;
    if (tri_mask_out_dev &&
        (st = FlagsToMaskAsync(flags, m, tri_mask_out_dev, s)))
        return st;
    return DownloadCount(w, n_triangles_out, s);
}

// RemoveDuplicatedTriangles (duplicated) or RemoveDegenerateTriangles.
int RemoveTriangles(bool duplicated, const void* triangles_dev, int64_t m,
                    int index_dtype, int64_t v, uint8_t* tri_mask_out_dev,
                    void* triangles_out_dev, int64_t* n_triangles_out,
                    hipStream_t s) {
    int st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(n_triangles_out, "null argument");
    O3DMI_REQUIRE(m == 0 || (triangles_dev && tri_mask_out_dev &&
                             triangles_out_dev),
                  "null argument");
    if (m == 0) {
        *n_triangles_out = 0;
        return O3DMI_OK;
    }
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    int32_t* flags = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    if (duplicated) {
        RepBuffers r;
        if ((st = AllocRep(pool, m, &r))) return st;
        if ((st = TripleRepAsync(tri, m, true, r.table, r.slots, r.rep, r.first,
                                 s)))
            return st;
        flags = r.first;
    } else {
        if ((st = pool.Alloc(&flags, sizeof(int32_t) * (size_t)m))) return st;
        if ((st = NonDegenerateFlagsAsync(tri, m, flags, s))) return st;
    }
    return KeepTriangles(pool, w, tri, m, index_dtype, flags, tri_mask_out_dev,
                         triangles_out_dev, n_triangles_out);
}

}  // namespace

namespace o3dmi {

int BuildAdjacency(PoolScratch& pool, const int32_t* tri, int64_t m, int64_t v,
                   bool pooled, int64_t capacity, int index_dtype,
                   void* neighbours_out_dev, MeshAdjacency* adj) {
    hipStream_t s = pool.s;
    const int64_t n3 = 3 * m;
    EdgeTable tb;
    void* scratch = nullptr;
    int32_t *flags = nullptr, *upper = nullptr, *lower = nullptr;
    int64_t *pos = nullptr, *upper_start = nullptr, *lower_start = nullptr;
    uint32_t *lo = nullptr, *hi = nullptr;
    struct Counts {
        unsigned long long n_self;
        long long n_edges;
    };
    Counts* counts = nullptr;
    const size_t slot_bytes = sizeof(uint32_t) * (size_t)n3;
    const size_t vertex_ints = sizeof(int32_t) * (size_t)v;
    int st = AllocEdgeTable(pool, n3, &tb);
    if (!st) st = pool.Alloc(&scratch, IncidenceScratchBytes(m, v));
    if (!st) st = pool.Alloc(&flags, sizeof(int32_t) * (size_t)n3);
    if (!st) st = pool.Alloc(&pos, sizeof(int64_t) * (size_t)n3);
    if (!st) st = pool.Alloc(&lo, slot_bytes);
    if (!st) st = pool.Alloc(&hi, slot_bytes);
    if (!st) st = pool.Alloc(&upper, vertex_ints);
    if (!st) st = pool.Alloc(&lower, vertex_ints);
    if (!st) st = pool.Alloc(&upper_start, sizeof(int64_t) * (size_t)v);
    if (!st) st = pool.Alloc(&lower_start, sizeof(int64_t) * (size_t)v);
    if (!st) st = pool.Alloc(&adj->row_splits, sizeof(int64_t) * ((size_t)v + 1));
    if (!st) st = pool.Alloc(&counts, 256);
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(Counts), s));
    O3DMI_HIP_CHECK(hipMemsetAsync(upper, 0, vertex_ints, s));
    O3DMI_HIP_CHECK(hipMemsetAsync(lower, 0, vertex_ints, s));
    if ((st = BuildEdgeTableAsync(tri, m, v, tb, scratch, s))) return st;
    if ((st = EdgeRunFlagsAsync(tb, n3, flags, &counts->n_self, s))) return st;
    if ((st = PrefixSumAsync(flags, n3, false, pos, (int64_t*)&counts->n_edges,
                             scratch, s)))
        return st;
    // the unique edges fit the table's own size: no wait before they are laid
    // out
    if ((st = UniqueEdgesAsync(tb, n3, flags, pos, lo, hi, upper, lower, s)))
        return st;
    if ((st = PrefixSumAsync(upper, v, false, upper_start, nullptr, scratch,
                             s)))
        return st;
    if ((st = PrefixSumAsync(lower, v, false, lower_start, nullptr, scratch,
                             s)))
        return st;
    Counts host;
    if ((st = Download(counts, &host, sizeof(host), s))) return st;
    const int64_t n_edges = (int64_t)host.n_edges;
    adj->n_entries = 2 * n_edges - (int64_t)host.n_self;
    adj->neighbours = nullptr;
    if ((st = AdjacencyRowsAsync(lower_start, upper_start, v, adj->n_entries,
                                 adj->row_splits, s)))
        return st;
    void* out = neighbours_out_dev;
    if (pooled) {
        if ((st = pool.Alloc(&adj->neighbours,
                             sizeof(int32_t) *
                                     (size_t)std::max<int64_t>(adj->n_entries,
                                                               1))))
            return st;
        out = adj->neighbours;
        index_dtype = O3DMI_I32;
    } else {
        if (capacity < 0) return O3DMI_OK;
        if (capacity < adj->n_entries)
            return CapacityError("adjacency list: capacity too small");
    }
    if (n_edges == 0) return O3DMI_OK;
    if ((st = AdjacencyUpperAsync(lo, hi, n_edges, adj->row_splits, lower,
                                  upper_start, index_dtype, out, s)))
        return st;
    // the edge table is done with: its arrays carry the (hi, lo) pairs
    if ((st = ByHiPairsAsync(lo, hi, n_edges, v, tb.hi, tb.lo, s))) return st;
    if ((st = SortPairsAsync(tb.hi, tb.lo, n_edges, BitsFor(v + 1), scratch,
                             s)))
        return st;
    return AdjacencyLowerAsync(tb.hi, tb.lo, n_edges, v, adj->row_splits,
                               lower_start, index_dtype, out, s);
}

}  // namespace o3dmi

extern "C" {

int o3dmi_trianglemesh_remove_duplicated_vertices(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        uint8_t* vertex_mask_out_dev, void* triangles_out_dev,
        int64_t* n_vertices_out, o3dmi_stream_t stream) {
    int st = CheckFloat(dtype);
    if (!st) st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(v < kRepMaxRows, "v out of range (< 2^30)");
    O3DMI_REQUIRE(n_vertices_out, "null argument");
    O3DMI_REQUIRE(v == 0 || (positions_dev && vertex_mask_out_dev),
                  "null argument");
    O3DMI_REQUIRE(m == 0 || (triangles_dev && triangles_out_dev),
                  "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if (m > 0 && (st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v,
                                     &tri)))
        return st;
    if (v == 0) {  // m == 0 too: a triangle list with v == 0 failed its check
        *n_vertices_out = 0;
        return O3DMI_OK;
    }
    RepBuffers r;
    int64_t* rank = nullptr;
    int64_t* vnew = nullptr;
    void* scratch = nullptr;
    if ((st = AllocRep(pool, v, &r))) return st;
    if ((st = pool.Alloc(&rank, sizeof(int64_t) * (size_t)v))) return st;
    if ((st = pool.Alloc(&vnew, sizeof(int64_t) * (size_t)v))) return st;
    if ((st = pool.Alloc(&scratch, ScanScratchBytes(v)))) return st;
    if ((st = VertexRepAsync(positions_dev, v, dtype, r.table, r.slots, r.rep,
                             r.first, s)))
        return st;
    if ((st = PrefixSumAsync(r.first, v, false, rank, (int64_t*)&w->count,
                             scratch, s)))
        return st;
    if ((st = RankOfRepAsync(r.rep, rank, v, vnew, s))) return st;
    if (m > 0 && (st = RemapTrianglesAsync(tri, m, nullptr, nullptr, vnew,
                                           index_dtype, triangles_out_dev, s)))
        return st;
    if ((st = FlagsToMaskAsync(r.first, v, vertex_mask_out_dev, s))) return st;
    return DownloadCount(w, n_vertices_out, s);
}

int o3dmi_trianglemesh_remove_duplicated_triangles(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        uint8_t* tri_mask_out_dev, void* triangles_out_dev,
        int64_t* n_triangles_out, o3dmi_stream_t stream) {
    return RemoveTriangles(true, triangles_dev, m, index_dtype, v,
                           tri_mask_out_dev, triangles_out_dev,
                           n_triangles_out, (hipStream_t)stream);
}

int o3dmi_trianglemesh_remove_degenerate_triangles(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        uint8_t* tri_mask_out_dev, void* triangles_out_dev,
        int64_t* n_triangles_out, o3dmi_stream_t stream) {
    return RemoveTriangles(false, triangles_dev, m, index_dtype, v,
                           tri_mask_out_dev, triangles_out_dev,
                           n_triangles_out, (hipStream_t)stream);
}

int o3dmi_trianglemesh_compute_adjacency_list(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        int64_t* row_splits_out_dev, void* neighbours_out_dev,
        int64_t capacity, int64_t* n_entries_out, o3dmi_stream_t stream) {
    int st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(n_entries_out, "null argument");
    O3DMI_REQUIRE(m == 0 || triangles_dev, "null argument");
    O3DMI_REQUIRE(capacity < 0 || row_splits_out_dev, "null argument");
    O3DMI_REQUIRE(capacity <= 0 || neighbours_out_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {  // every list is empty
        *n_entries_out = 0;
        if (capacity >= 0) {
            O3DMI_HIP_CHECK(hipMemsetAsync(row_splits_out_dev, 0,
                                           sizeof(int64_t) * ((size_t)v + 1),
                                           s));
            O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        }
        return O3DMI_OK;
    }
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    MeshAdjacency adj = {};
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    st = BuildAdjacency(pool, tri, m, v, false, capacity, index_dtype,
                        neighbours_out_dev, &adj);
    if (st == O3DMI_OK || st == O3DMI_ERR_CAPACITY)
        *n_entries_out = adj.n_entries;
    if (st || capacity < 0) return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(row_splits_out_dev, adj.row_splits,
                                   sizeof(int64_t) * ((size_t)v + 1),
                                   hipMemcpyDeviceToDevice, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

int o3dmi_trianglemesh_simplify_vertex_clustering(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        double voxel_size, int contraction, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, void* triangles_out_dev,
        int64_t* n_vertices_out, int64_t* n_triangles_out,
        o3dmi_stream_t stream) {
    int st = CheckFloat(dtype);
    if (!st) st = CheckSizes(v, m, index_dtype);
    if (!st)
        st = CheckVertexAttrs(dtype, attr_dtype, normals_dev, colors_dev,
                              normals_out_dev, colors_out_dev);
    if (st) return st;
    O3DMI_REQUIRE(v < kRepMaxRows, "v out of range (< 2^30)");
    O3DMI_REQUIRE(voxel_size > 0.0 && voxel_size - voxel_size == 0.0,
                  "voxel_size <= 0.0");
    O3DMI_REQUIRE(contraction == 0 || contraction == 1,
                  "contraction must be 0 (Average) or 1 (Quadric)");
    O3DMI_REQUIRE(n_vertices_out && n_triangles_out, "null argument");
    O3DMI_REQUIRE(v == 0 || (positions_dev && positions_out_dev),
                  "null argument");
    O3DMI_REQUIRE(m == 0 || (triangles_dev && triangles_out_dev),
                  "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if (m > 0 && (st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v,
                                     &tri)))
        return st;
    if (v == 0) {  // m == 0 too: a triangle list with v == 0 failed its check
        *n_vertices_out = *n_triangles_out = 0;
        return O3DMI_OK;
    }
    if ((st = RequireFinite(positions_dev, v, dtype, w, s))) return st;

    // the voxel grid
    double* bound_scratch = nullptr;
    double* bound_dev = nullptr;
    double bound[6];
    if ((st = pool.Alloc(&bound_scratch,
                         sizeof(double) * MinMaxScratchDoubles())))
        return st;
    if ((st = MinMaxBoundAsync(positions_dev, v, dtype, bound_scratch,
                               &bound_dev, s)))
        return st;
    if ((st = Download(bound_dev, bound, sizeof(bound), s))) return st;
    double min_bound[3], extent = 0;
    for (int k = 0; k < 3; ++k) {
        min_bound[k] = bound[k] - voxel_size * 0.5;
        const double max_bound = bound[3 + k] + voxel_size * 0.5;
        extent = k == 0 ? max_bound - min_bound[k]
                        : std::max(extent, max_bound - min_bound[k]);
    }
    O3DMI_REQUIRE(!(voxel_size * (double)INT_MAX < extent),
                  "voxel_size is too small.");

    // clusters numbered by their first vertex
    int32_t* vox = nullptr;
    RepBuffers r;
    int64_t *rank = nullptr, *vnew = nullptr;
    void* scratch = nullptr;
    const int64_t sort_n = std::max(v, m);
    if ((st = pool.Alloc(&vox, sizeof(int32_t) * 3 * (size_t)v))) return st;
    if ((st = AllocRep(pool, std::max(v, m), &r))) return st;
    if ((st = pool.Alloc(&rank, sizeof(int64_t) * (size_t)v))) return st;
    if ((st = pool.Alloc(&vnew, sizeof(int64_t) * (size_t)v))) return st;
    if ((st = pool.Alloc(&scratch,
                         std::max({SortPairsScratchBytes(sort_n),
                                   ScanScratchBytes(sort_n),
                                   m > 0 ? IncidenceScratchBytes(m, v)
                                         : (size_t)0}))))
        return st;
    if ((st = VoxelIndicesAsync(positions_dev, v, dtype, min_bound, voxel_size,
                                vox, s)))
        return st;
    if ((st = TripleRepAsync(vox, v, false, r.table, RepTableSlots(v), r.rep,
                             r.first, s)))
        return st;
    if ((st = PrefixSumAsync(r.first, v, false, rank, (int64_t*)&w->count,
                             scratch, s)))
        return st;
    if ((st = RankOfRepAsync(r.rep, rank, v, vnew, s))) return st;
    int64_t n_clusters = 0;
    if ((st = DownloadCount(w, &n_clusters, s))) return st;

    // member lists in ascending old index
    uint32_t *keys = nullptr, *members = nullptr;
    int32_t *counts = nullptr, *long_list = nullptr;
    int64_t* start = nullptr;
    if ((st = pool.Alloc(&keys, sizeof(uint32_t) * (size_t)v))) return st;
    if ((st = pool.Alloc(&members, sizeof(uint32_t) * (size_t)v))) return st;
    if ((st = pool.Alloc(&counts, sizeof(int32_t) * (size_t)n_clusters)))
        return st;
    if ((st = pool.Alloc(&start, sizeof(int64_t) * (size_t)n_clusters)))
        return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(counts, 0,
                                   sizeof(int32_t) * (size_t)n_clusters, s));
    if ((st = AllocLongList(pool, n_clusters, &long_list))) return st;
    if ((st = ClusterPairsAsync(vnew, v, keys, members, counts, s))) return st;
    if ((st = SortPairsAsync(keys, members, v, BitsFor(n_clusters), scratch,
                             s)))
        return st;
    if ((st = PrefixSumAsync(counts, n_clusters, false, start, nullptr,
                             scratch, s)))
        return st;

    ClusterIO io = {};
    io.positions = positions_dev;
    io.normals = normals_dev;
    io.colors = colors_dev;
    io.members = members;
    io.start = start;
    io.counts = counts;
    io.positions_out = positions_out_dev;
    io.normals_out = normals_out_dev;
    io.colors_out = colors_out_dev;
    if (contraction == 1 && m > 0) {
        double *plane = nullptr, *area = nullptr;
        io.quadric = true;
        if ((st = AllocCornerTable(pool, m, v, &io.corners))) return st;
        if ((st = pool.Alloc(&plane, sizeof(double) * 4 * (size_t)m)))
            return st;
        if ((st = pool.Alloc(&area, sizeof(double) * (size_t)m))) return st;
        if ((st = BuildCornerTableAsync(tri, m, v, io.corners, scratch, s)))
            return st;
        if ((st = TrianglePlanesAsync(positions_dev, dtype, tri, m, plane, s)))
            return st;
        if ((st = TriangleAreasF64Async(positions_dev, dtype, tri, m, area, s)))
            return st;
        io.plane = plane;
        io.area = area;
    }
    if ((st = ContractClustersAsync(io, n_clusters, dtype, long_list, s)))
        return st;

    // the triangles that still join three clusters, once each
    int64_t n_triangles = 0;
    if (m > 0) {
        int32_t* mapped = nullptr;
        if ((st = pool.Alloc(&mapped, sizeof(int32_t) * 3 * (size_t)m)))
            return st;
        if ((st = MapClusterTrianglesAsync(tri, m, vnew, mapped, s))) return st;
        if ((st = TripleRepAsync(mapped, m, false, r.table, RepTableSlots(m),
                                 r.rep, r.first, s)))
            return st;
        if ((st = KeepTriangles(pool, w, mapped, m, index_dtype, r.first,
                                nullptr, triangles_out_dev, &n_triangles)))
            return st;
    } else {
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    }
    *n_vertices_out = n_clusters;
    *n_triangles_out = n_triangles;
    return O3DMI_OK;
}

}  // extern "C"
