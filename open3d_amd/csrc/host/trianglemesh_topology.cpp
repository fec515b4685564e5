// Host drivers of the mesh topology and intersection queries: legacy
// EulerPoincareCharacteristic, IsEdgeManifold, GetNonManifoldVertices,
// IsOrientable / OrientTriangles, GetSelfIntersectingTriangles /
// IsSelfIntersecting, IsIntersecting, IsWatertight and GetVolume
// (geometry/TriangleMesh.cpp:1016-1135, 1212-1246, 1272-1457) as chains of
// the incidence tables, the union-find, the scan, the pair sort and the mesh
// BVH. Arguments are checked before anything is allocated, the triangle
// indices on the device before anything is written; the kernels are in
// trianglemesh_topology.hip.
#include <algorithm>
#include <cmath>

#include "../pointcloud_sample.h"
#include "../scan.h"
#include "../sort.h"
#include "../trianglemesh_clean.h"
#include "../trianglemesh_topology.h"
#include "o3d_mi355x_host.h"
#include "trianglemesh_call.h"

using namespace o3dmi;

namespace {

// The device cells of one call, zeroed once; every step has its own.
struct Cells {
    int orient_bad;
    int finite_bad;
    int overflow;
    int pad;
    unsigned long long n_flagged;
    unsigned long long n_self;
    unsigned long long n_pairs;
    unsigned long long visits[2];
    long long n_vertices;
};

// A checked triangle list (m >= 1) and what the steps of a call share.
struct Call {
    PoolScratch& pool;
    const int32_t* tri;
    int64_t m, v;
    Cells* cells = nullptr;
    EdgeTable edges = {};
    void* scratch = nullptr;  // IncidenceScratchBytes(m, v)
    int32_t* flags = nullptr;  // max(3 m, v) ints
    Call(PoolScratch& p, const int32_t* t, int64_t m_, int64_t v_)
        : pool(p), tri(t), m(m_), v(v_) {}
};

int Begin(Call* c) {
    int st = c->pool.Alloc(&c->cells, 256);
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(c->cells, 0, sizeof(Cells), c->pool.s));
    return O3DMI_OK;
}

// The edge table, built once a call.
int NeedEdges(Call* c) {
    if (c->edges.lo) return O3DMI_OK;
    int st = AllocEdgeTable(c->pool, 3 * c->m, &c->edges);
    if (!st)
        st = c->pool.Alloc(&c->scratch, IncidenceScratchBytes(c->m, c->v));
    if (!st)
        st = c->pool.Alloc(&c->flags,
                           sizeof(int32_t) *
                                   (size_t)std::max(3 * c->m, c->v));
    if (st) return st;
    return BuildEdgeTableAsync(c->tri, c->m, c->v, c->edges, c->scratch,
                               c->pool.s);
}

// The number of (lo, hi) runs of the edge table. One wait.
int CountEdges(Call* c, int64_t* n_out) {
    hipStream_t s = c->pool.s;
    int st = NeedEdges(c);
    if (st) return st;
    if ((st = EdgeRunFlagsAsync(c->edges, 3 * c->m, c->flags,
                                &c->cells->n_self, s)))
        return st;
    if ((st = CountFlagsAsync(c->flags, 3 * c->m, &c->cells->n_flagged, s)))
        return st;
    unsigned long long n = 0;
    if ((st = Download(&c->cells->n_flagged, &n, sizeof(n), s))) return st;
    *n_out = (int64_t)n;
    return O3DMI_OK;
}

// IsEdgeManifold. One wait.
int EdgeManifold(Call* c, bool allow_boundary, int* out) {
    hipStream_t s = c->pool.s;
    int st = NeedEdges(c);
    if (st) return st;
    if ((st = NonManifoldFlagsAsync(c->edges, 3 * c->m, allow_boundary,
                                    c->flags, s)))
        return st;
    if ((st = CountFlagsAsync(c->flags, 3 * c->m, &c->cells->n_flagged, s)))
        return st;
    unsigned long long n = 0;
    if ((st = Download(&c->cells->n_flagged, &n, sizeof(n), s))) return st;
    *out = n == 0;
    return O3DMI_OK;
}

// GetNonManifoldVertices with the count / fill protocol (capacity < 0 only
// counts). One wait before the fill.
int NonManifoldVertices(Call* c, int index_dtype, void* out_dev,
                        int64_t capacity, int64_t* n_out) {
    hipStream_t s = c->pool.s;
    CornerTable corners;
    int* parent = nullptr;
    int32_t* long_list = nullptr;
    int64_t* pos = nullptr;
    int st = NeedEdges(c);
    if (!st) st = AllocCornerTable(c->pool, c->m, c->v, &corners);
    if (!st) st = c->pool.Alloc(&parent, sizeof(int) * 3 * (size_t)c->m);
    if (!st) st = c->pool.Alloc(&pos, sizeof(int64_t) * (size_t)c->v);
    if (!st) st = AllocLongList(c->pool, c->v, &long_list);
    if (st) return st;
    if ((st = BuildCornerTableAsync(c->tri, c->m, c->v, corners, c->scratch,
                                    s)))
        return st;
    if ((st = NonManifoldVertexFlagsAsync(c->tri, c->m, c->v, c->edges,
                                          corners, parent, long_list, c->flags,
                                          s)))
        return st;
    if ((st = PrefixSumAsync(c->flags, c->v, false, pos,
                             (int64_t*)&c->cells->n_vertices, c->scratch, s)))
        return st;
    long long n = 0;
    if ((st = Download(&c->cells->n_vertices, &n, sizeof(n), s))) return st;
    *n_out = (int64_t)n;
    if (capacity < 0 || n == 0) return O3DMI_OK;
    if (capacity < n)
        return CapacityError("non-manifold vertices: capacity too small");
    if ((st = EmitFlaggedAsync(c->flags, pos, c->v, index_dtype, out_dev, s)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

// OrientTriangles; triangles_out_dev may be NULL. One wait.
int Orient(Call* c, int index_dtype, void* triangles_out_dev,
           int* orientable_out) {
    hipStream_t s = c->pool.s;
    int* parent = nullptr;
    int32_t* flip = nullptr;
    int st = NeedEdges(c);
    if (!st) st = c->pool.Alloc(&parent, sizeof(int) * 2 * (size_t)c->m);
    if (!st) st = c->pool.Alloc(&flip, sizeof(int32_t) * (size_t)c->m);
    if (st) return st;
    if ((st = OrientFlipsAsync(c->tri, c->m, c->edges, parent, flip,
                               &c->cells->orient_bad, s)))
        return st;
    if (triangles_out_dev &&
        (st = WriteOrientedAsync(c->tri, c->m, flip, &c->cells->orient_bad,
                                 index_dtype, triangles_out_dev, s)))
        return st;
    int bad = 0;
    if ((st = Download(&c->cells->orient_bad, &bad, sizeof(bad), s)))
        return st;
    *orientable_out = !bad;
    return O3DMI_OK;
}

// Refuses a mesh with a referenced coordinate that is not finite as given or
// as a float (one launch, one download), as o3dmi_mesh_bvh_create does.
int RequireReferencedFinite(const void* positions_dev, int dtype,
                            const int32_t* tri, int64_t m, int* bad_dev,
                            hipStream_t s) {
    int st = CheckReferencedFiniteAsync(positions_dev, dtype, tri, m, bad_dev,
                                        s);
    if (st) return st;
    int bad = 0;
    if ((st = Download(bad_dev, &bad, sizeof(bad), s))) return st;
    O3DMI_REQUIRE(!bad,
                  "non-finite coordinate: run RemoveNonFinitePoints first");
    return O3DMI_OK;
}

// The tree over the triangles of a mesh whose referenced positions are finite,
// everything from the pool.
int BuildTree(PoolScratch& pool, const void* positions_dev, int64_t v,
              int dtype, const int32_t* tri, int64_t m, MeshBvhView* view) {
    hipStream_t s = pool.s;
    const float* narrow = (const float*)positions_dev;
    if (dtype == O3DMI_F64) {
        float* p = nullptr;
        int st = pool.Alloc(&p, sizeof(float) * 3 * (size_t)v);
        if (st) return st;
        if ((st = NarrowAsync((const double*)positions_dev, 3 * v, O3DMI_F32,
                              p, s)))
            return st;
        narrow = p;
    }
    BvhNode* nodes = nullptr;
    BvhLeaf* leaves = nullptr;
    float* scene = nullptr;
    void* scratch = nullptr;
    int st = O3DMI_OK;
    if (m > 1) st = pool.Alloc(&nodes, sizeof(BvhNode) * (size_t)(m - 1));
    if (!st) st = pool.Alloc(&leaves, sizeof(BvhLeaf) * (size_t)m);
    if (!st) st = pool.Alloc(&scene, 256);
    if (!st) st = pool.Alloc(&scratch, MeshBvhBuildScratchBytes(m));
    if (st) return st;
    *view = MeshBvhView();
    view->nodes = nodes;
    view->leaves = leaves;
    view->m = m;
    return BuildMeshBvhAsync(narrow, tri, m, nodes, leaves, scene, scratch, s);
}

// What a traversal left in the cells. One wait.
int TraversalResult(Call* c, int64_t* n_out, unsigned long long* visits_out) {
    Cells host;
    int st = Download(c->cells, &host, sizeof(host), c->pool.s);
    if (st) return st;
    if (host.overflow) {
        SetLastError("intersections: traversal stack overflow");
        return O3DMI_ERR_INTERNAL;
    }
    *n_out = (int64_t)host.n_pairs;
    if (visits_out) {
        visits_out[0] = host.visits[0];
        visits_out[1] = host.visits[1];
    }
    return O3DMI_OK;
}

// GetSelfIntersectingTriangles (kIntersectList, the count / fill protocol) or
// IsSelfIntersecting (kIntersectAny: *n_out is 0 / 1).
int SelfIntersections(Call* c, const void* positions_dev, int dtype,
                      IntersectKind kind, int index_dtype, void* pairs_out_dev,
                      int64_t capacity, int64_t* n_out,
                      unsigned long long* visits_out) {
    hipStream_t s = c->pool.s;
    int st = RequireReferencedFinite(positions_dev, dtype, c->tri, c->m,
                                     &c->cells->finite_bad, s);
    if (st) return st;
    IntersectTarget target = {};
    if ((st = BuildTree(c->pool, positions_dev, c->v, dtype, c->tri, c->m,
                        &target.bvh)))
        return st;
    target.positions = positions_dev;
    target.dtype = dtype;
    target.tri = c->tri;
    IntersectQuery query = {true, positions_dev, dtype, c->tri, c->m};
    uint32_t *is = nullptr, *js = nullptr;
    void* sort_scratch = nullptr;
    const int64_t room = kind == kIntersectList ? capacity : 0;
    if (room > 0) {
        if ((st = c->pool.Alloc(&is, sizeof(uint32_t) * (size_t)room)))
            return st;
        if ((st = c->pool.Alloc(&js, sizeof(uint32_t) * (size_t)room)))
            return st;
        if ((st = c->pool.Alloc(&sort_scratch, SortPairsScratchBytes(room))))
            return st;
    }
    if ((st = MeshIntersectAsync(kind, query, target, is, js, room,
                                 &c->cells->n_pairs, &c->cells->overflow,
                                 visits_out ? c->cells->visits : nullptr, s)))
        return st;
    int64_t n = 0;
    if ((st = TraversalResult(c, &n, visits_out))) return st;
    *n_out = kind == kIntersectAny ? (n != 0) : n;
    if (kind == kIntersectAny || capacity < 0 || n == 0) return O3DMI_OK;
    if (capacity < n)
        return CapacityError("self-intersecting triangles: capacity too small");
    // the pairs are distinct: stably by j, then by i, is ascending (i, j)
    const int bits = BitsFor(c->m);
    if ((st = SortPairsAsync(js, is, n, bits, sort_scratch, s))) return st;
    if ((st = SortPairsAsync(is, js, n, bits, sort_scratch, s))) return st;
    if ((st = WritePairsAsync(is, js, n, index_dtype, pairs_out_dev, s)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

// IsWatertight: the cheap tests first.
int Watertight(Call* c, const void* positions_dev, int dtype, int* out) {
    int ok = 0;
    int st = EdgeManifold(c, false, &ok);
    if (st) return st;
    *out = 0;
    if (!ok) return O3DMI_OK;
    int64_t n = 0;
    if ((st = NonManifoldVertices(c, O3DMI_I32, nullptr, -1, &n))) return st;
    if (n) return O3DMI_OK;
    if ((st = SelfIntersections(c, positions_dev, dtype, kIntersectAny,
                                O3DMI_I32, nullptr, -1, &n, nullptr)))
        return st;
    *out = n == 0;
    return O3DMI_OK;
}

int CheckIndexArgs(const void* triangles_dev, int64_t m, int index_dtype,
                   int64_t v) {
    const int st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(m == 0 || triangles_dev, "null argument");
    return O3DMI_OK;
}

int CheckMeshArgs(const void* positions_dev, int64_t v, int dtype,
                  const void* triangles_dev, int64_t m, int index_dtype) {
    int st = CheckFloat(dtype);
    if (!st) st = CheckSizes(v, m, index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(m == 0 || (positions_dev && triangles_dev), "null argument");
    return O3DMI_OK;
}

// The scaffold of a call on a non-empty triangle list: the checked list and
// the zeroed cells, then `body`.
template <typename Body>
int WithTriangles(const void* triangles_dev, int64_t m, int index_dtype,
                  int64_t v, hipStream_t s, Body body) {
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    int st = AllocWords(pool, &w);
    if (st) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    Call call(pool, tri, m, v);
    if ((st = Begin(&call))) return st;
    return body(&call);
}

// The closed box test of IntersectionTest::AABBAABB on {min xyz, max xyz}.
bool BoundsOverlap(const double a[6], const double b[6]) {
    for (int k = 0; k < 3; ++k)
        if (a[3 + k] < b[k] || a[k] > b[3 + k]) return false;
    return true;
}

}  // namespace

extern "C" {

int o3dmi_trianglemesh_euler_poincare_characteristic(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        int64_t* characteristic_out, o3dmi_stream_t stream) {
    int st = CheckIndexArgs(triangles_dev, m, index_dtype, v);
    if (st) return st;
    O3DMI_REQUIRE(characteristic_out, "null argument");
    if (m == 0) {
        *characteristic_out = v;
        return O3DMI_OK;
    }
    return WithTriangles(triangles_dev, m, index_dtype, v, (hipStream_t)stream,
                         [&](Call* c) -> int {
                             int64_t e = 0;
                             const int st2 = CountEdges(c, &e);
                             if (st2) return st2;
                             *characteristic_out = v + m - e;
                             return (int)O3DMI_OK;
                         });
}

int o3dmi_trianglemesh_is_edge_manifold(const void* triangles_dev, int64_t m,
                                        int index_dtype, int64_t v,
                                        int allow_boundary_edges,
                                        int* manifold_out,
                                        o3dmi_stream_t stream) {
    int st = CheckIndexArgs(triangles_dev, m, index_dtype, v);
    if (st) return st;
    O3DMI_REQUIRE(manifold_out, "null argument");
    if (m == 0) {
        *manifold_out = 1;
        return O3DMI_OK;
    }
    return WithTriangles(triangles_dev, m, index_dtype, v, (hipStream_t)stream,
                         [&](Call* c) -> int {
                             return EdgeManifold(c, allow_boundary_edges != 0,
                                                 manifold_out);
                         });
}

int o3dmi_trianglemesh_get_non_manifold_vertices(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        void* vertices_out_dev, int64_t capacity, int64_t* n_vertices_out,
        o3dmi_stream_t stream) {
    int st = CheckIndexArgs(triangles_dev, m, index_dtype, v);
    if (st) return st;
    O3DMI_REQUIRE(n_vertices_out, "null argument");
    O3DMI_REQUIRE(capacity <= 0 || vertices_out_dev, "null argument");
    if (m == 0) {
        *n_vertices_out = 0;
        return O3DMI_OK;
    }
    return WithTriangles(triangles_dev, m, index_dtype, v, (hipStream_t)stream,
                         [&](Call* c) -> int {
                             return NonManifoldVertices(c, index_dtype,
                                                        vertices_out_dev,
                                                        capacity,
                                                        n_vertices_out);
                         });
}

int o3dmi_trianglemesh_orient_triangles(const void* triangles_dev, int64_t m,
                                        int index_dtype, int64_t v,
                                        void* triangles_out_dev,
                                        int* orientable_out,
                                        o3dmi_stream_t stream) {
    int st = CheckIndexArgs(triangles_dev, m, index_dtype, v);
    if (st) return st;
    O3DMI_REQUIRE(orientable_out, "null argument");
    if (m == 0) {
        *orientable_out = 1;
        return O3DMI_OK;
    }
    return WithTriangles(triangles_dev, m, index_dtype, v, (hipStream_t)stream,
                         [&](Call* c) -> int {
                             return Orient(c, index_dtype, triangles_out_dev,
                                           orientable_out);
                         });
}

int o3dmi_trianglemesh_get_self_intersecting_triangles(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        void* pairs_out_dev, int64_t capacity, int64_t* n_pairs_out,
        o3dmi_stream_t stream) {
    int st = CheckMeshArgs(positions_dev, v, dtype, triangles_dev, m,
                           index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(n_pairs_out, "null argument");
    O3DMI_REQUIRE(capacity <= 0 || pairs_out_dev, "null argument");
    O3DMI_REQUIRE(capacity < (1ll << 31), "capacity out of range (< 2^31)");
    if (m == 0) {
        *n_pairs_out = 0;
        return O3DMI_OK;
    }
    return WithTriangles(triangles_dev, m, index_dtype, v, (hipStream_t)stream,
                         [&](Call* c) -> int {
                             return SelfIntersections(
                                     c, positions_dev, dtype, kIntersectList,
                                     index_dtype, pairs_out_dev, capacity,
                                     n_pairs_out, nullptr);
                         });
}

int o3dmi_trianglemesh_is_self_intersecting(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        int* intersecting_out, o3dmi_stream_t stream) {
    int st = CheckMeshArgs(positions_dev, v, dtype, triangles_dev, m,
                           index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(intersecting_out, "null argument");
    if (m == 0) {
        *intersecting_out = 0;
        return O3DMI_OK;
    }
    return WithTriangles(triangles_dev, m, index_dtype, v, (hipStream_t)stream,
                         [&](Call* c) -> int {
                             int64_t n = 0;
                             const int st2 = SelfIntersections(
                                     c, positions_dev, dtype, kIntersectAny,
                                     index_dtype, nullptr, -1, &n, nullptr);
                             if (st2) return st2;
                             *intersecting_out = n != 0;
                             return (int)O3DMI_OK;
                         });
}

int o3dmi_internal_trianglemesh_self_intersections(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype, int kind,
        int64_t* n_out, unsigned long long* visits_out,
        o3dmi_stream_t stream) {
    int st = CheckMeshArgs(positions_dev, v, dtype, triangles_dev, m,
                           index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(n_out && visits_out, "null argument");
    O3DMI_REQUIRE(kind == kIntersectList || kind == kIntersectAny,
                  "kind must be 0 (list) or 1 (any)");
    visits_out[0] = visits_out[1] = 0;
    if (m == 0) {
        *n_out = 0;
        return O3DMI_OK;
    }
    return WithTriangles(triangles_dev, m, index_dtype, v, (hipStream_t)stream,
                         [&](Call* c) -> int {
                             return SelfIntersections(
                                     c, positions_dev, dtype,
                                     (IntersectKind)kind, index_dtype, nullptr,
                                     -1, n_out, visits_out);
                         });
}

int o3dmi_trianglemesh_is_intersecting(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* other_positions_dev, int64_t other_v, int other_dtype,
        const void* other_triangles_dev, int64_t other_m,
        int other_index_dtype, int* intersecting_out, o3dmi_stream_t stream) {
    int st = CheckMeshArgs(positions_dev, v, dtype, triangles_dev, m,
                           index_dtype);
    if (!st)
        st = CheckMeshArgs(other_positions_dev, other_v, other_dtype,
                           other_triangles_dev, other_m, other_index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(intersecting_out, "null argument");
    *intersecting_out = 0;
    if (m == 0 || other_m == 0) return O3DMI_OK;  // no pair of triangles
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    Words *w = nullptr, *other_w = nullptr;
    const int32_t *tri = nullptr, *other_tri = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = AllocWords(pool, &other_w))) return st;
    if ((st = LoadTriangles(pool, w, triangles_dev, m, index_dtype, v, &tri)))
        return st;
    if ((st = LoadTriangles(pool, other_w, other_triangles_dev, other_m,
                            other_index_dtype, other_v, &other_tri)))
        return st;
    Call call(pool, tri, m, v);
    if ((st = Begin(&call))) return st;
    // w->bad and other_w->bad are still zero: the lists passed their checks
    if ((st = RequireReferencedFinite(positions_dev, dtype, tri, m, &w->bad,
                                      s)))
        return st;
    if ((st = RequireReferencedFinite(other_positions_dev, other_dtype,
                                      other_tri, other_m, &other_w->bad, s)))
        return st;

    // GetMinBound / GetMaxBound of both meshes, over all their vertices
    double *bound_scratch = nullptr, *other_scratch = nullptr;
    double *bound_dev = nullptr, *other_bound_dev = nullptr;
    double bound[6], other_bound[6];
    const size_t bound_bytes = sizeof(double) * MinMaxScratchDoubles();
    if ((st = pool.Alloc(&bound_scratch, bound_bytes))) return st;
    if ((st = pool.Alloc(&other_scratch, bound_bytes))) return st;
    if ((st = MinMaxBoundAsync(positions_dev, v, dtype, bound_scratch,
                               &bound_dev, s)))
        return st;
    if ((st = MinMaxBoundAsync(other_positions_dev, other_v, other_dtype,
                               other_scratch, &other_bound_dev, s)))
        return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(bound, bound_dev, sizeof(bound),
                                   hipMemcpyDeviceToHost, s));
    if ((st = Download(other_bound_dev, other_bound, sizeof(other_bound), s)))
        return st;
    if (!BoundsOverlap(bound, other_bound)) return O3DMI_OK;

    IntersectTarget target = {};
    if ((st = BuildTree(pool, other_positions_dev, other_v, other_dtype,
                        other_tri, other_m, &target.bvh)))
        return st;
    target.positions = other_positions_dev;
    target.dtype = other_dtype;
    target.tri = other_tri;
    IntersectQuery query = {false, positions_dev, dtype, tri, m};
    if ((st = MeshIntersectAsync(kIntersectAny, query, target, nullptr,
                                 nullptr, 0, &call.cells->n_pairs,
                                 &call.cells->overflow, nullptr, s)))
        return st;
    int64_t n = 0;
    if ((st = TraversalResult(&call, &n, nullptr))) return st;
    *intersecting_out = n != 0;
    return O3DMI_OK;
}

int o3dmi_trianglemesh_is_watertight(const void* positions_dev, int64_t v,
                                     int dtype, const void* triangles_dev,
                                     int64_t m, int index_dtype,
                                     int* watertight_out,
                                     o3dmi_stream_t stream) {
    int st = CheckMeshArgs(positions_dev, v, dtype, triangles_dev, m,
                           index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(watertight_out, "null argument");
    if (m == 0) {
        *watertight_out = 1;
        return O3DMI_OK;
    }
    return WithTriangles(triangles_dev, m, index_dtype, v, (hipStream_t)stream,
                         [&](Call* c) -> int {
                             return Watertight(c, positions_dev, dtype,
                                               watertight_out);
                         });
}

int o3dmi_trianglemesh_get_volume(const void* positions_dev, int64_t v,
                                  int dtype, const void* triangles_dev,
                                  int64_t m, int index_dtype,
                                  double* volume_out, o3dmi_stream_t stream) {
    int st = CheckMeshArgs(positions_dev, v, dtype, triangles_dev, m,
                           index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(volume_out, "null argument");
    if (m == 0) {
        *volume_out = 0.0;
        return O3DMI_OK;
    }
    return WithTriangles(
            triangles_dev, m, index_dtype, v, (hipStream_t)stream,
            [&](Call* c) -> int {
                hipStream_t s = c->pool.s;
                int ok = 0;
                int st2 = Watertight(c, positions_dev, dtype, &ok);
                if (st2) return st2;
                O3DMI_REQUIRE(ok,
                              "The mesh is not watertight, and the volume "
                              "cannot be computed.");
                if ((st2 = Orient(c, index_dtype, nullptr, &ok))) return st2;
                O3DMI_REQUIRE(ok,
                              "The mesh is not orientable, and the volume "
                              "cannot be computed.");
                double *terms = nullptr, *sums = nullptr;
                if ((st2 = c->pool.Alloc(&terms, sizeof(double) * (size_t)m)))
                    return st2;
                if ((st2 = c->pool.Alloc(
                             &sums,
                             sizeof(double) * RunSumScratchDoubles(m))))
                    return st2;
                if ((st2 = TetraVolumesAsync(positions_dev, dtype, c->tri, m,
                                             terms, s)))
                    return st2;
                const double* total = nullptr;
                if ((st2 = RunSumTreeAsync(terms, m, O3DMI_F64, sums, &total,
                                           s)))
                    return st2;
                double volume = 0;
                if ((st2 = Download(total, &volume, sizeof(volume), s)))
                    return st2;
                *volume_out = std::fabs(volume);
                return (int)O3DMI_OK;
            });
}

}  // extern "C"
