// Host driver of ClipPlane / SlicePlane (t/geometry/TriangleMesh.cpp:649-716):
// the checks, the signed values, the classification, the numbering of the
// slots that cross, then the emit. A call waits once for the triangle range
// check, once for the finiteness of every attribute and signed value (one
// flag, one download), once for the compaction totals and once for the number
// of distinct points, whose sort needs the number of crossing slots on the
// host. Slice does the last two per contour and keeps of each contour only
// its point records and its lines, which are written out once every contour
// is counted and the capacities are checked. The kernels are in
// trianglemesh_clip.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../scan.h"
#include "../sort.h"
#include "../trianglemesh_clip.h"
#include "o3d_mi355x_host.h"
#include "trianglemesh_call.h"

using namespace o3dmi;

namespace {

// What clip and slice take alike.
struct CutInput {
    const void* positions;
    int64_t v;
    int dtype;
    const void* normals;
    const void* colors;
    int attr_dtype;
    const void* triangles;
    int64_t m;
    int index_dtype;
    const double* point;
    const double* normal;
};

// The totals a call downloads, on the device.
struct Totals {
    long long pieces;  // output triangles / lines
    long long old;     // old vertices kept (clip)
    long long used;    // slots that cross
    long long points;  // distinct points of those slots
};

// The dtype and size checks, from the sizes alone.
int CheckInput(const CutInput& c, int64_t max_m, const char* max_m_msg) {
    int st = CheckFloat(c.dtype);
    if (!st) st = CheckSizes(c.v, c.m, c.index_dtype);
    if (st) return st;
    O3DMI_REQUIRE(c.m <= max_m, max_m_msg);
    O3DMI_REQUIRE(c.v + 3 * c.m < (1ll << 31),
                  "v + 3 m out of range (< 2^31 points)");
    if ((c.normals || c.colors) && c.attr_dtype != c.dtype)
        return Unsupported(
                "vertex normals and colours must have the position dtype");
    O3DMI_REQUIRE(c.point && c.normal, "null argument");
    for (int k = 0; k < 3; ++k)
        O3DMI_REQUIRE(std::isfinite(c.point[k]) && std::isfinite(c.normal[k]),
                      "point and normal must be finite");
    O3DMI_REQUIRE(c.normal[0] != 0 || c.normal[1] != 0 || c.normal[2] != 0,
                  "normal must not be (0, 0, 0)");
    O3DMI_REQUIRE(c.v == 0 || c.positions, "null argument");
    O3DMI_REQUIRE(c.m == 0 || c.triangles, "null argument");
    O3DMI_REQUIRE(c.v > 0 || c.m == 0, "triangle index outside [0, v)");
    return O3DMI_OK;
}

// The checked triangle list and the signed values of a mesh with v >= 1; one
// wait for the finiteness of every attribute and value.
int LoadInput(PoolScratch& pool, const CutInput& c, const int32_t** tri,
              double** s_dev) {
    hipStream_t s = pool.s;
    Words* w = nullptr;
    int st = AllocWords(pool, &w);
    if (st) return st;
    if (c.m > 0 && (st = LoadTriangles(pool, w, c.triangles, c.m,
                                       c.index_dtype, c.v, tri)))
        return st;
    if ((st = pool.Alloc(s_dev, sizeof(double) * (size_t)c.v))) return st;
    const void* ins[3] = {c.positions, c.normals, c.colors};
    for (int a = 0; a < 3; ++a)
        if (ins[a] && (st = CheckFiniteAsync(ins[a], c.v, c.dtype, &w->bad, s)))
            return st;
    CutPlane plane;
    for (int k = 0; k < 3; ++k) {
        plane.o[k] = c.point[k];
        plane.n[k] = c.normal[k];
    }
    if ((st = PlaneValuesAsync(c.positions, c.v, c.dtype, plane, *s_dev,
                               &w->bad, s)))
        return st;
    int bad = 0;
    if ((st = Download(&w->bad, &bad, sizeof(bad), s))) return st;
    O3DMI_REQUIRE(!bad,
                  "non-finite position, normal, colour or signed value");
    return O3DMI_OK;
}

CutAttrs AttrsOf(const CutInput& c, void* positions_out, void* normals_out,
                 void* colors_out) {
    const void* ins[3] = {c.positions, c.normals, c.colors};
    void* outs[3] = {positions_out, normals_out, colors_out};
    CutAttrs at = {};
    for (int a = 0; a < 3; ++a) {
        if (!ins[a]) continue;
        at.in[at.n_attrs] = ins[a];
        at.out[at.n_attrs++] = outs[a];
    }
    return at;
}

// The points of the flagged slots, numbered: n_points, and with `ids` their
// records (from `keep`) and the point of every compacted slot (from `tmp`, as
// everything else here).
struct Ranked {
    int64_t n_points;
    SubdivEdges points;
    int32_t* id_by_pos;
};
int RankPoints(PoolScratch& tmp, PoolScratch& keep, Totals* tot,
               const int32_t* tri, int64_t m, int64_t v, const double* s_dev,
               double c, const int32_t* slot_used, const int64_t* slot_pos,
               int64_t n_used, bool ids, Ranked* out) {
    hipStream_t s = tmp.s;
    *out = {};
    if (n_used == 0) return O3DMI_OK;
    uint32_t* slot_of = nullptr;
    EdgeTable table;  // a "slot" is a compact position
    EdgeRunScans scans;
    void* scratch = nullptr;
    int st = tmp.Alloc(&slot_of, sizeof(uint32_t) * (size_t)n_used);
    if (!st) st = AllocEdgeTable(tmp, n_used, &table);
    if (!st)
        st = tmp.Alloc(&scratch, std::max(SortPairsScratchBytes(n_used),
                                          ScanScratchBytes(n_used)));
    if (st) return st;
    if ((st = CompactSlotsAsync(slot_used, slot_pos, 3 * m, slot_of, s)))
        return st;
    if ((st = SortSlotKeysAsync(tri, s_dev, c, slot_of, n_used, BitsFor(v),
                                table.lo, table.hi, table.slot, scratch, s)))
        return st;
    if ((st = CountEdgeRuns(tmp, table, n_used, ids, false, scratch,
                            &tot->points, &scans, &out->n_points)))
        return st;
    if (!ids) return O3DMI_OK;
    return NumberEdgeRuns(tmp, keep, table, n_used, scans, out->n_points, 0,
                          nullptr, &out->points, &out->id_by_pos);
}

// ---- clip ---------------------------------------------------------------------------
struct ClipOutput {
    void* positions;
    void* normals;
    void* colors;
    int64_t vertex_capacity;
    void* triangles;
    int64_t triangle_capacity;
    void* triangle_source;
    void* vertex_source;
    double* vertex_t;
    int64_t* n_vertices;
    int64_t* n_triangles;
};

int ClipPlane(const CutInput& c, const ClipOutput& o, hipStream_t s) {
    int st = CheckInput(c, 1ll << 28, "m out of range (<= 2^28 triangles)");
    if (st) return st;
    O3DMI_REQUIRE(o.n_vertices && o.n_triangles, "null argument");
    O3DMI_REQUIRE(!o.vertex_source == !o.vertex_t,
                  "vertex_source_out and vertex_t_out go together");
    const bool count_only = o.vertex_capacity < 0;
    if (o.vertex_capacity > 0) {
        O3DMI_REQUIRE(o.positions, "null argument");
        O3DMI_REQUIRE(!c.normals || o.normals,
                      "null argument: normals given, no output for them");
        O3DMI_REQUIRE(!c.colors || o.colors,
                      "null argument: colours given, no output for them");
    }
    if (!count_only && o.triangle_capacity > 0)
        O3DMI_REQUIRE(o.triangles, "null argument");
    if (c.v == 0) {
        *o.n_vertices = *o.n_triangles = 0;
        return O3DMI_OK;
    }

    const int64_t v = c.v, m = c.m, n3 = 3 * m;
    PoolScratch pool(s);
    const int32_t* tri = nullptr;
    double* s_dev = nullptr;
    if ((st = LoadInput(pool, c, &tri, &s_dev))) return st;
    if (m == 0) {
        *o.n_vertices = *o.n_triangles = 0;
        return O3DMI_OK;
    }

    Totals* tot = nullptr;
    int32_t *pieces = nullptr, *slot_used = nullptr, *vertex_used = nullptr;
    int64_t *piece_pos = nullptr, *slot_pos = nullptr, *old_id = nullptr;
    void* scratch = nullptr;
    st = pool.Alloc(&tot, 256);
    if (!st) st = pool.Alloc(&pieces, sizeof(int32_t) * (size_t)m);
    if (!st) st = pool.Alloc(&slot_used, sizeof(int32_t) * (size_t)n3);
    if (!st) st = pool.Alloc(&vertex_used, sizeof(int32_t) * (size_t)v);
    if (!st) st = pool.Alloc(&piece_pos, sizeof(int64_t) * (size_t)m);
    if (!st) st = pool.Alloc(&slot_pos, sizeof(int64_t) * (size_t)n3);
    if (!st) st = pool.Alloc(&old_id, sizeof(int64_t) * (size_t)v);
    if (!st) st = pool.Alloc(&scratch, ScanScratchBytes(std::max(n3, v)));
    if (st) return st;
    O3DMI_HIP_CHECK(
            hipMemsetAsync(vertex_used, 0, sizeof(int32_t) * (size_t)v, s));
    if ((st = ClipClassifyAsync(tri, m, s_dev, pieces, slot_used, vertex_used,
                                s)))
        return st;
    if ((st = PrefixSumAsync(pieces, m, false, piece_pos,
                             (int64_t*)&tot->pieces, scratch, s)))
        return st;
    if ((st = PrefixSumAsync(vertex_used, v, false, old_id,
                             (int64_t*)&tot->old, scratch, s)))
        return st;
    if ((st = PrefixSumAsync(slot_used, n3, false, slot_pos,
                             (int64_t*)&tot->used, scratch, s)))
        return st;
    Totals h = {};
    if ((st = Download(tot, &h, sizeof(h), s))) return st;

    Ranked rk;
    if ((st = RankPoints(pool, pool, tot, tri, m, v, s_dev, 0., slot_used,
                         slot_pos, h.used, !count_only, &rk)))
        return st;
    const int64_t n_v = h.old + rk.n_points, n_t = h.pieces;
    *o.n_vertices = n_v;
    *o.n_triangles = n_t;
    if (count_only) return O3DMI_OK;
    if (o.vertex_capacity < n_v)
        return CapacityError("clip_plane: vertex capacity too small");
    if (o.triangle_capacity < n_t)
        return CapacityError("clip_plane: triangle capacity too small");
    if (n_t == 0) return O3DMI_OK;

    const CutAttrs attrs = AttrsOf(c, o.positions, o.normals, o.colors);
    if ((st = ClipOldVerticesAsync(vertex_used, old_id, v, c.dtype, attrs,
                                   c.index_dtype, o.vertex_source, o.vertex_t,
                                   s)))
        return st;
    if (rk.n_points > 0 &&
        (st = CutPointsAsync(rk.points, rk.n_points, h.old, s_dev, 0., c.dtype,
                             attrs, c.index_dtype, o.vertex_source, o.vertex_t,
                             s)))
        return st;
    if ((st = ClipEmitAsync(tri, m, s_dev, piece_pos, old_id, h.old, slot_pos,
                            rk.id_by_pos, c.index_dtype, o.triangles,
                            o.triangle_source, s)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

// ---- slice --------------------------------------------------------------------------
struct SliceOutput {
    void* points;
    void* normals;
    void* colors;
    int64_t point_capacity;
    void* lines;
    int64_t line_capacity;
    void* line_triangle;
    int32_t* line_contour;
    void* point_source;
    double* point_t;
    int64_t* n_points;
    int64_t* n_lines;
};

// The per-triangle tables of one contour, reused from contour to contour.
struct SliceTables {
    Totals* tot;
    int32_t* lines;
    int32_t* slot_used;
    int64_t* line_pos;
    int64_t* slot_pos;
    void* scratch;
};

// What a contour leaves behind for the emit: its counts, its place in the
// outputs and, unless only counting, its point records and its lines as (t,
// from, to) with the points numbered within the contour.
struct ContourCut {
    int64_t n_lines, n_points;
    int64_t line_base, point_base;
    SubdivEdges points;
    int32_t* rec;
};

// One contour: its lines, the slots of their ends, the points of those slots.
// Nothing of the caller's is written here, since the capacity check needs the
// counts of every contour: what the emit needs is small (the crossing
// triangles only) and stays in `pool`; the rest goes back at the contour's end.
int SliceContour(PoolScratch& pool, const SliceTables& tb, const int32_t* tri,
                 int64_t m, int64_t v, const double* s_dev, double c,
                 bool records, ContourCut* cut) {
    hipStream_t s = pool.s;
    PoolScratch tmp(s);
    int st = SliceClassifyAsync(tri, m, s_dev, c, tb.lines, tb.slot_used, s);
    if (st) return st;
    if ((st = PrefixSumAsync(tb.lines, m, false, tb.line_pos,
                             (int64_t*)&tb.tot->pieces, tb.scratch, s)))
        return st;
    if ((st = PrefixSumAsync(tb.slot_used, 3 * m, false, tb.slot_pos,
                             (int64_t*)&tb.tot->used, tb.scratch, s)))
        return st;
    Totals h = {};
    if ((st = Download(tb.tot, &h, sizeof(h), s))) return st;
    Ranked rk;
    if ((st = RankPoints(tmp, pool, tb.tot, tri, m, v, s_dev, c, tb.slot_used,
                         tb.slot_pos, h.used, records, &rk)))
        return st;
    cut->n_lines = h.pieces;
    cut->n_points = rk.n_points;
    cut->points = rk.points;
    cut->rec = nullptr;
    if (!records || h.pieces == 0) return O3DMI_OK;
    if ((st = pool.Alloc(&cut->rec, sizeof(int32_t) * 3 * (size_t)h.pieces)))
        return st;
    return SliceLineRecordsAsync(tri, m, s_dev, c, tb.lines, tb.line_pos,
                                 tb.slot_pos, rk.id_by_pos, cut->rec, s);
}

int SlicePlane(const CutInput& c, const double* contours, int64_t n_contours,
               const SliceOutput& o, hipStream_t s) {
    O3DMI_REQUIRE(n_contours >= 0, "the number of contour values is negative");
    int st = CheckInput(
            c,
            n_contours > 0 ? kMeshMaxTriangles / n_contours
                           : kMeshMaxTriangles,
            "K m out of range (<= 2^29 lines)");
    if (st) return st;
    O3DMI_REQUIRE(n_contours == 0 || contours, "null argument");
    for (int64_t k = 0; k < n_contours; ++k)
        O3DMI_REQUIRE(std::isfinite(contours[k]),
                      "contour values must be finite");
    O3DMI_REQUIRE(o.n_points && o.n_lines, "null argument");
    O3DMI_REQUIRE(!o.point_source == !o.point_t,
                  "point_source_out and point_t_out go together");
    const bool count_only = o.point_capacity < 0;
    if (o.point_capacity > 0) {
        O3DMI_REQUIRE(o.points, "null argument");
        O3DMI_REQUIRE(!c.normals || o.normals,
                      "null argument: normals given, no output for them");
        O3DMI_REQUIRE(!c.colors || o.colors,
                      "null argument: colours given, no output for them");
    }
    if (!count_only && o.line_capacity > 0)
        O3DMI_REQUIRE(o.lines, "null argument");
    if (c.v == 0) {
        *o.n_points = *o.n_lines = 0;
        return O3DMI_OK;
    }

    const int64_t v = c.v, m = c.m, n3 = 3 * m;
    PoolScratch pool(s);
    const int32_t* tri = nullptr;
    double* s_dev = nullptr;
    if ((st = LoadInput(pool, c, &tri, &s_dev))) return st;
    if (m == 0 || n_contours == 0) {
        *o.n_points = *o.n_lines = 0;
        return O3DMI_OK;
    }

    SliceTables tb = {};
    st = pool.Alloc(&tb.tot, 256);
    if (!st) st = pool.Alloc(&tb.lines, sizeof(int32_t) * (size_t)m);
    if (!st) st = pool.Alloc(&tb.slot_used, sizeof(int32_t) * (size_t)n3);
    if (!st) st = pool.Alloc(&tb.line_pos, sizeof(int64_t) * (size_t)m);
    if (!st) st = pool.Alloc(&tb.slot_pos, sizeof(int64_t) * (size_t)n3);
    if (!st) st = pool.Alloc(&tb.scratch, ScanScratchBytes(n3));
    if (st) return st;

    std::vector<ContourCut> cuts((size_t)n_contours);
    int64_t n_lines = 0, n_points = 0;
    for (int64_t k = 0; k < n_contours; ++k) {
        ContourCut& cut = cuts[(size_t)k];
        if ((st = SliceContour(pool, tb, tri, m, v, s_dev, contours[k],
                               !count_only, &cut)))
            return st;
        cut.line_base = n_lines;
        cut.point_base = n_points;
        n_lines += cut.n_lines;
        n_points += cut.n_points;
    }
    *o.n_points = n_points;
    *o.n_lines = n_lines;
    if (count_only) return O3DMI_OK;
    if (o.point_capacity < n_points)
        return CapacityError("slice_plane: point capacity too small");
    if (o.line_capacity < n_lines)
        return CapacityError("slice_plane: line capacity too small");

    const CutAttrs attrs = AttrsOf(c, o.points, o.normals, o.colors);
    for (int64_t k = 0; k < n_contours; ++k) {
        const ContourCut& cut = cuts[(size_t)k];
        if (cut.n_lines == 0) continue;  // then no point either
        if ((st = CutPointsAsync(cut.points, cut.n_points, cut.point_base,
                                 s_dev, contours[k], c.dtype, attrs,
                                 c.index_dtype, o.point_source, o.point_t, s)))
            return st;
        if ((st = SliceLinesOutAsync(cut.rec, cut.n_lines, cut.line_base,
                                     cut.point_base, (int)k, c.index_dtype,
                                     o.lines, o.line_triangle, o.line_contour,
                                     s)))
            return st;
    }
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

}  // namespace

extern "C" {

int o3dmi_trianglemesh_clip_plane(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const double* point, const double* normal, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, int64_t vertex_capacity,
        void* triangles_out_dev, int64_t triangle_capacity,
        void* triangle_source_out_dev, void* vertex_source_out_dev,
        double* vertex_t_out_dev, int64_t* n_vertices_out,
        int64_t* n_triangles_out, o3dmi_stream_t stream) {
    return ClipPlane({positions_dev, v, dtype, normals_dev, colors_dev,
                      attr_dtype, triangles_dev, m, index_dtype, point, normal},
                     {positions_out_dev, normals_out_dev, colors_out_dev,
                      vertex_capacity, triangles_out_dev, triangle_capacity,
                      triangle_source_out_dev, vertex_source_out_dev,
                      vertex_t_out_dev, n_vertices_out, n_triangles_out},
                     (hipStream_t)stream);
}

int o3dmi_trianglemesh_slice_plane(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const double* point, const double* normal,
        const double* contour_values, int64_t n_contours, void* points_out_dev,
        void* normals_out_dev, void* colors_out_dev, int64_t point_capacity,
        void* lines_out_dev, int64_t line_capacity,
        void* line_triangle_out_dev, int32_t* line_contour_out_dev,
        void* point_source_out_dev, double* point_t_out_dev,
        int64_t* n_points_out, int64_t* n_lines_out, o3dmi_stream_t stream) {
    return SlicePlane({positions_dev, v, dtype, normals_dev, colors_dev,
                       attr_dtype, triangles_dev, m, index_dtype, point,
                       normal},
                      contour_values, n_contours,
                      {points_out_dev, normals_out_dev, colors_out_dev,
                       point_capacity, lines_out_dev, line_capacity,
                       line_triangle_out_dev, line_contour_out_dev,
                       point_source_out_dev, point_t_out_dev, n_points_out,
                       n_lines_out},
                      (hipStream_t)stream);
}

}  // extern "C"
