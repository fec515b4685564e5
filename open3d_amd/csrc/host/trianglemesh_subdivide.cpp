// Host driver of SubdivideMidpoint / SubdivideLoop (legacy geometry/
// TriangleMeshSubdivide.cpp): the checks, the index side of every iteration
// first (topology never depends on coordinates, so the count call does no
// attribute work beyond the finiteness gate), then the float64 attributes
// iteration by iteration and one narrowing at the end. Per iteration the host
// waits once for the number of edges; Loop's adjacency build waits once more.
// What an iteration needs only while it is built comes from a pool of its
// own; what the attribute phase reads later (the edge records) stays in the
// call's pool. The kernels are in trianglemesh_subdivide.hip.
#include <algorithm>
#include <vector>

#include "../scan.h"
#include "../trianglemesh_clean.h"
#include "../trianglemesh_subdivide.h"
#include "o3d_mi355x_host.h"
#include "trianglemesh_call.h"

using namespace o3dmi;

namespace o3dmi {

// The numbering chain of trianglemesh_subdivide.h, shared with ClipPlane /
// SlicePlane (host/trianglemesh_clip.cpp), whose "edges" are the distinct cut
// points. The one wait of the chain is at the end of the first half, so a
// caller can stop after the count or check a capacity before anything of its
// own is written.
int CountEdgeRuns(PoolScratch& tmp, const EdgeTable& table, int64_t n_slots,
                  bool number, bool triangles, void* scratch_dev,
                  long long* total_dev, EdgeRunScans* scans,
                  int64_t* n_runs_out) {
    hipStream_t s = tmp.s;
    *scans = {};
    int32_t* by_slot = nullptr;
    const size_t slot_bytes = sizeof(uint32_t) * (size_t)n_slots;
    const size_t scan_bytes = sizeof(int64_t) * (size_t)n_slots;
    int st = tmp.Alloc(&scans->head, slot_bytes);
    if (!st) st = tmp.Alloc(&by_slot, slot_bytes);
    if (!st) st = tmp.Alloc(&scans->rank_by_slot, scan_bytes);
    if (!st) st = tmp.Alloc(&scans->q_incl, scan_bytes);
    if (!st && triangles) st = tmp.Alloc(&scans->distinct, slot_bytes);
    if (!st && triangles) st = tmp.Alloc(&scans->distinct_incl, scan_bytes);
    if (st) return st;
    if ((st = EdgeSlotFlagsAsync(table, n_slots, scans->head, by_slot,
                                 scans->distinct, s)))
        return st;
    if ((st = PrefixSumAsync(by_slot, n_slots, false, scans->rank_by_slot,
                             (int64_t*)total_dev, scratch_dev, s)))
        return st;
    long long n_runs = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&n_runs, total_dev, sizeof(n_runs),
                                   hipMemcpyDeviceToHost, s));
    if (number && (st = PrefixSumAsync(scans->head, n_slots, true,
                                       scans->q_incl, nullptr, scratch_dev, s)))
        return st;
    if (number && triangles &&
        (st = PrefixSumAsync(scans->distinct, n_slots, true,
                             scans->distinct_incl, nullptr, scratch_dev, s)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    *n_runs_out = n_runs;
    return O3DMI_OK;
}

int NumberEdgeRuns(PoolScratch& tmp, PoolScratch& keep, const EdgeTable& table,
                   int64_t n_slots, const EdgeRunScans& scans, int64_t n_runs,
                   int64_t id_base, const int32_t* tri, SubdivEdges* edges,
                   int32_t** id_by_slot) {
    hipStream_t s = tmp.s;
    const bool triangles = scans.distinct != nullptr;
    *edges = {};
    const size_t run_bytes = sizeof(uint32_t) * (size_t)n_runs;
    const size_t slot_bytes = sizeof(uint32_t) * (size_t)n_slots;
    int st = keep.Alloc(&edges->lo, run_bytes);
    if (!st) st = keep.Alloc(&edges->hi, run_bytes);
    if (!st) st = keep.Alloc(&edges->rank, run_bytes);
    if (!st) st = keep.Alloc(&edges->head, run_bytes + sizeof(int32_t));
    if (!st && triangles) st = keep.Alloc(&edges->triangles, run_bytes);
    if (!st && triangles) st = keep.Alloc(&edges->opposite, slot_bytes);
    if (!st) st = tmp.Alloc(id_by_slot, slot_bytes);
    if (st) return st;
    if ((st = EdgeRecordsAsync(table, n_slots, scans.head, scans.q_incl,
                               scans.rank_by_slot, n_runs, *edges, s)))
        return st;
    return SlotVertexIdsAsync(table, n_slots, scans.q_incl, *edges, id_base,
                              scans.distinct, tri, *id_by_slot, s);
}

}  // namespace o3dmi

namespace {

struct SubdivideCall {
    const void* positions;
    int64_t v;
    int dtype;
    const void* normals;
    const void* colors;
    int attr_dtype;
    const void* triangles;
    int64_t m;
    int index_dtype;
    int iterations;
    void* positions_out;
    void* normals_out;
    void* colors_out;
    int64_t vertex_capacity;
    void* triangles_out;
    int64_t* n_vertices_out;
    int64_t* n_triangles_out;
    hipStream_t s;
};

// One iteration's input and what the attribute phase needs of it.
struct Level {
    const int32_t* tri;
    int64_t m;
    int64_t v;
    int64_t n_edges;
    SubdivEdges edges;
};

// The index side of one iteration: the edge records of lv->tri and, unless
// `last` and count_only, the refined list (int32 into *tri_next from the
// call's pool, or for the last iteration into out_dev in the index dtype).
// Between the edge count and anything written, `last` checks the capacity.
int RefineLevel(PoolScratch& pool, Words* w, const SubdivideCall& c, bool loop,
                bool last, Level* lv, int32_t** tri_next) {
    hipStream_t s = pool.s;
    const int64_t m = lv->m, v = lv->v, n3 = 3 * m;
    PoolScratch tmp(s);
    EdgeTable tb;
    void* scratch = nullptr;
    EdgeRunScans scans;
    int32_t* new_id = nullptr;
    int st = AllocEdgeTable(tmp, n3, &tb);
    if (!st)
        st = tmp.Alloc(&scratch, std::max(IncidenceScratchBytes(m, v),
                                          ScanScratchBytes(n3)));
    if (st) return st;
    if ((st = BuildEdgeTableAsync(lv->tri, m, v, tb, scratch, s))) return st;
    if ((st = CountEdgeRuns(tmp, tb, n3, true, loop, scratch, &w->total,
                            &scans, &lv->n_edges)))
        return st;
    const int64_t n_edges = lv->n_edges;
    if (last) {
        *c.n_vertices_out = v + n_edges;
        *c.n_triangles_out = 4 * m;
        if (c.vertex_capacity < 0) return O3DMI_OK;
        if (c.vertex_capacity < v + n_edges)
            return CapacityError("subdivide: vertex capacity too small");
    }

    SubdivEdges& ed = lv->edges;
    if ((st = NumberEdgeRuns(tmp, pool, tb, n3, scans, n_edges, v, lv->tri,
                             &ed, &new_id)))
        return st;
    if (loop &&
        (st = EdgeTriangleCountsAsync(ed, n_edges, scans.distinct_incl, s)))
        return st;
    if (last)
        return EmitSubdividedAsync(lv->tri, m, new_id, c.index_dtype,
                                   c.triangles_out, s);
    if ((st = pool.Alloc(tri_next, sizeof(int32_t) * 12 * (size_t)m)))
        return st;
    return EmitSubdividedAsync(lv->tri, m, new_id, O3DMI_I32, *tri_next, s);
}

// Loop's attribute pass of one iteration: the adjacency of the level's list,
// its boundary flags, the old vertices, the new vertices.
int LoopLevel(PoolScratch& pool, const Level& lv, const SubdivAttrs& attrs) {
    hipStream_t s = pool.s;
    const int64_t v = lv.v, n_edges = lv.n_edges;
    PoolScratch tmp(s);
    MeshAdjacency adj = {};
    uint8_t* boundary = nullptr;
    int32_t *long_vertices = nullptr, *long_edges = nullptr;
    int st = BuildAdjacency(tmp, lv.tri, lv.m, v, true, 0, O3DMI_I32, nullptr,
                            &adj);
    if (!st)
        st = tmp.Alloc(&boundary,
                       (size_t)std::max<int64_t>(adj.n_entries, 1));
    if (!st) st = AllocLongList(tmp, v, &long_vertices);
    if (!st) st = AllocLongList(tmp, n_edges, &long_edges);
    if (st) return st;
    if ((st = BoundaryFlagsAsync(lv.edges, n_edges, adj.row_splits,
                                 adj.neighbours, boundary, s)))
        return st;
    if ((st = LongListsAsync(adj.row_splits, v, long_vertices, s))) return st;
    if ((st = LongEdgeRunsAsync(lv.edges, n_edges, long_edges, s))) return st;
    if ((st = LoopOldVerticesAsync(adj.row_splits, adj.neighbours, boundary, v,
                                   attrs, long_vertices, s)))
        return st;
    return LoopNewVerticesAsync(lv.edges, n_edges, v, attrs, long_edges, s);
}

int Subdivide(const SubdivideCall& c, bool loop) {
    int st = CheckFloat(c.dtype);
    if (!st) st = CheckSizes(c.v, c.m, c.index_dtype);
    if (st) return st;
    if ((c.normals || c.colors) && c.attr_dtype != c.dtype)
        return Unsupported(
                "vertex normals and colours must have the position dtype");
    O3DMI_REQUIRE(c.n_vertices_out && c.n_triangles_out, "null argument");
    O3DMI_REQUIRE(c.v == 0 || c.positions, "null argument");
    O3DMI_REQUIRE(c.m == 0 || c.triangles, "null argument");
    const bool count_only = c.vertex_capacity < 0;
    const int64_t v = c.v, m = c.m;
    const int n_iter = m > 0 && c.iterations > 0 ? c.iterations : 0;
    // 4^n m triangles and at most v + (4^n - 1) m vertices (three new ones
    // per triangle and iteration), before anything is allocated
    int64_t m_out = m;
    for (int i = 0; i < n_iter; ++i) {
        m_out *= 4;
        O3DMI_REQUIRE(m_out <= kMeshMaxTriangles,
                      "4^n m out of range (<= 2^29 triangles)");
    }
    O3DMI_REQUIRE(v + (m_out - m) < (1ll << 31),
                  "v + (4^n - 1) m out of range (< 2^31 vertices)");
    if (c.vertex_capacity > 0) {  // 0 rows hold no vertex: nothing is written
        O3DMI_REQUIRE(v == 0 || c.positions_out, "null argument");
        O3DMI_REQUIRE(m == 0 || c.triangles_out, "null argument");
        O3DMI_REQUIRE(!c.normals || c.normals_out,
                      "null argument: normals given, no output for them");
        O3DMI_REQUIRE(!c.colors || c.colors_out,
                      "null argument: colours given, no output for them");
    }
    if (v == 0) {  // m == 0 too, or the range check below would refuse it
        O3DMI_REQUIRE(m == 0, "triangle index outside [0, v)");
        *c.n_vertices_out = *c.n_triangles_out = 0;
        return O3DMI_OK;
    }

    hipStream_t s = c.s;
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if (m > 0 && (st = LoadTriangles(pool, w, c.triangles, m, c.index_dtype, v,
                                     &tri)))
        return st;
    const void* ins[3] = {c.positions, c.normals, c.colors};
    void* outs[3] = {c.positions_out, c.normals_out, c.colors_out};
    for (int a = 0; a < 3; ++a)
        if (ins[a] && (st = RequireFinite(ins[a], v, c.dtype, w, s)))
            return st;

    if (n_iter == 0) {  // upstream's loop runs zero times: a copy
        *c.n_vertices_out = v;
        *c.n_triangles_out = m;
        if (count_only) return O3DMI_OK;
        if (c.vertex_capacity < v)
            return CapacityError("subdivide: vertex capacity too small");
        const size_t row_bytes = 3 * ElemSize(c.dtype) * (size_t)v;
        for (int a = 0; a < 3; ++a)
            if (ins[a])
                O3DMI_HIP_CHECK(hipMemcpyAsync(outs[a], ins[a], row_bytes,
                                               hipMemcpyDeviceToDevice, s));
        if (m > 0)
            O3DMI_HIP_CHECK(hipMemcpyAsync(
                    c.triangles_out, c.triangles,
                    3 * (c.index_dtype == O3DMI_I64 ? 8 : 4) * (size_t)m,
                    hipMemcpyDeviceToDevice, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        return O3DMI_OK;
    }

    // the index side of every iteration
    std::vector<Level> levels((size_t)n_iter);
    Level cur = {tri, m, v, 0, {}};
    for (int i = 0; i < n_iter; ++i) {
        const bool last = i == n_iter - 1;
        int32_t* tri_next = nullptr;
        if ((st = RefineLevel(pool, w, c, loop, last, &cur, &tri_next)))
            return st;
        levels[(size_t)i] = cur;
        cur = {tri_next, 4 * cur.m, cur.v + cur.n_edges, 0, {}};
    }
    if (count_only) return O3DMI_OK;
    const int64_t v_out = cur.v;

    // the attributes in float64: Midpoint appends in place, Loop ping-pongs
    double* buf[kMaxSubdivAttrs][2] = {};
    int attr_of[kMaxSubdivAttrs], n_attrs = 0;
    const size_t buf_bytes = sizeof(double) * 3 * (size_t)v_out;
    for (int a = 0; a < 3; ++a) {
        if (!ins[a]) continue;
        if ((st = pool.Alloc(&buf[n_attrs][0], buf_bytes))) return st;
        if (loop && (st = pool.Alloc(&buf[n_attrs][1], buf_bytes))) return st;
        if ((st = WidenAsync(ins[a], 3 * v, c.dtype, buf[n_attrs][0], s)))
            return st;
        attr_of[n_attrs++] = a;
    }
    int side = 0;
    for (const Level& lv : levels) {
        SubdivAttrs attrs = {};
        attrs.n_attrs = n_attrs;
        for (int k = 0; k < n_attrs; ++k) {
            attrs.prev[k] = buf[k][side];
            attrs.next[k] = buf[k][loop ? side ^ 1 : side];
        }
        if (loop) {
            if ((st = LoopLevel(pool, lv, attrs))) return st;
            side ^= 1;
        } else if ((st = MidpointVerticesAsync(lv.edges, lv.n_edges, lv.v,
                                               attrs, s))) {
            return st;
        }
    }
    for (int k = 0; k < n_attrs; ++k)
        if ((st = NarrowAsync(buf[k][side], 3 * v_out, c.dtype,
                              outs[attr_of[k]], s)))
            return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

}  // namespace

extern "C" {

int o3dmi_trianglemesh_subdivide_midpoint(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        int number_of_iterations, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, int64_t vertex_capacity,
        void* triangles_out_dev, int64_t* n_vertices_out,
        int64_t* n_triangles_out, o3dmi_stream_t stream) {
    return Subdivide({positions_dev, v, dtype, normals_dev, colors_dev,
                      attr_dtype, triangles_dev, m, index_dtype,
                      number_of_iterations, positions_out_dev, normals_out_dev,
                      colors_out_dev, vertex_capacity, triangles_out_dev,
                      n_vertices_out, n_triangles_out, (hipStream_t)stream},
                     false);
}

int o3dmi_trianglemesh_subdivide_loop(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        int number_of_iterations, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, int64_t vertex_capacity,
        void* triangles_out_dev, int64_t* n_vertices_out,
        int64_t* n_triangles_out, o3dmi_stream_t stream) {
    return Subdivide({positions_dev, v, dtype, normals_dev, colors_dev,
                      attr_dtype, triangles_dev, m, index_dtype,
                      number_of_iterations, positions_out_dev, normals_out_dev,
                      colors_out_dev, vertex_capacity, triangles_out_dev,
                      n_vertices_out, n_triangles_out, (hipStream_t)stream},
                     true);
}

}  // extern "C"
