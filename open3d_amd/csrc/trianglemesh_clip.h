// Private seam between trianglemesh_clip.hip (the kernels of ClipPlane /
// SlicePlane, t/geometry/TriangleMesh.cpp:649-716, which upstream hands to
// VTK on a host copy) and host/trianglemesh_clip.cpp (the C ABI and the
// driver). Every launcher is stream-ordered and waits for nothing; `tri` is
// the checked int32 triangle list of trianglemesh.h, `s` the signed value of
// every vertex (PlaneValuesAsync), `c` the contour value (0 for clip).
//
// THE RULES both calls share (the C header states them in full). Vertex i is
// inside iff s[i] >= c. A triangle with one vertex inside is rotated, winding
// kept, so that this vertex is first; one with two inside so that the outside
// one is last: (a, b, c), with the edge slots ab = 3 t + r, bc = 3 t + (r + 1)
// % 3, ca = 3 t + (r + 2) % 3 for the rotation r. The cut point of a crossing
// edge with the inside end u is VERTEX u when s[u] == c, else the point of the
// unordered edge (lo, hi). A point is named by its key: (u, u) or (lo, hi),
// lo < hi; two uses are one point iff their keys agree. An output triangle or
// line that names a point twice is dropped and numbers nothing.
//
// NUMBERING. The kept pieces flag the slots whose points they use (clip: the
// edge points only, its old vertices are numbered apart). The flagged slots
// are compacted in slot order, sorted stably by key, and the point of a run of
// equal keys gets the rank of the run's first entry, its lowest slot, among
// all first entries: SubdivideMidpoint's numbering over the slots that cross
// instead of all 3 m.
#pragma once

#include "common.h"
#include "trianglemesh.h"
#include "trianglemesh_subdivide.h"

namespace o3dmi {

// The threads of a workgroup of every kernel here (tests name it).
constexpr int kClipBlock = kBlock;

struct CutPlane {
    double o[3];
    double n[3];
};

// s[i] = ((n.x (x - o.x) + n.y (y - o.y)) + n.z (z - o.z)) from the position
// widened; *bad_dev |= 1 when one is not finite.
int PlaneValuesAsync(const void* positions_dev, int64_t v, int dtype,
                     const CutPlane& plane, double* s_dev, int* bad_dev,
                     hipStream_t s);

// Clip, a thread per triangle: pieces[t] = the number of kept output
// triangles (0, 1, 2), slot_used[3 t + k] = 1 where a kept piece names the
// edge point of that slot (every word is written), vertex_used[u] = 1 for the
// old vertices kept pieces name (over flags zeroed by the caller).
int ClipClassifyAsync(const int32_t* tri, int64_t m, const double* s_dev,
                      int32_t* pieces_dev, int32_t* slot_used_dev,
                      int32_t* vertex_used_dev, hipStream_t s);
// Slice, a thread per triangle: lines[t] = 1 when the triangle's line is kept,
// slot_used[3 t + k] = 1 for the slots of its two ends (vertex points too).
int SliceClassifyAsync(const int32_t* tri, int64_t m, const double* s_dev,
                       double c, int32_t* lines_dev, int32_t* slot_used_dev,
                       hipStream_t s);

// slot_of[pos[e]] = e for the flagged slots (pos: the exclusive scan).
int CompactSlotsAsync(const int32_t* slot_used_dev, const int64_t* pos_dev,
                      int64_t n_slots, uint32_t* slot_of_dev, hipStream_t s);
// The compacted slots in ascending (lo, hi, slot) of their point keys: order
// {n} holds compact positions, lo / hi the keys of order[j]. scratch:
// SortPairsScratchBytes(n).
int SortSlotKeysAsync(const int32_t* tri, const double* s_dev, double c,
                      const uint32_t* slot_of_dev, int64_t n, int key_bits,
                      uint32_t* lo_dev, uint32_t* hi_dev, uint32_t* order_dev,
                      void* scratch_dev, hipStream_t s);
// From here the numbering is SubdivideMidpoint's, by its launchers
// (trianglemesh_subdivide.h) over the table {lo, hi, slot = order}:
// EdgeSlotFlagsAsync (run heads, in sorted order and per compact position),
// EdgeRecordsAsync (the distinct points in key order as SubdivEdges: lo, hi and
// rank, the point's number within its contour) and SlotVertexIdsAsync with v =
// 0 (the point of every compacted slot).

// ---- emit -------------------------------------------------------------------------
// The {rows,3} attributes of a call in the position dtype: positions, then
// normals and colours where given.
constexpr int kMaxCutAttrs = 3;
struct CutAttrs {
    int n_attrs;
    const void* in[kMaxCutAttrs];
    void* out[kMaxCutAttrs];
};
// Row base + rank[q] of every output for the point q < n_points: vertex lo
// copied bit for bit when lo == hi, else t = (c - s[lo]) / (s[hi] - s[lo]) and
// x[lo] + t * (x[hi] - x[lo]) per component in float64, narrowed on the store.
// source_out {rows,2} in the index dtype and t_out {rows} (both or neither):
// (lo, hi) and t, 0 for a vertex point.
int CutPointsAsync(const SubdivEdges& points, int64_t n_points, int64_t base,
                   const double* s_dev, double c, int dtype,
                   const CutAttrs& attrs, int index_dtype, void* source_out_dev,
                   double* t_out_dev, hipStream_t s);
// Clip: row old_id[u] of every output = row u for the flagged old vertices,
// bit for bit; source (u, u), t 0.
int ClipOldVerticesAsync(const int32_t* vertex_used_dev,
                         const int64_t* old_id_dev, int64_t v, int dtype,
                         const CutAttrs& attrs, int index_dtype,
                         void* source_out_dev, double* t_out_dev,
                         hipStream_t s);
// Clip: rows piece_pos[t] .. of triangles_out (index dtype) and
// triangle_source_out (may be NULL) for the kept pieces of triangle t: (a, ab,
// ca) with one inside, (a, b, bc) then (a, bc, ca) with two, the triangle
// itself with three. An old vertex u is old_id[u]; the edge point of slot e is
// n_old + id_by_pos[slot_pos[e]] (id_by_pos: SlotVertexIdsAsync's).
int ClipEmitAsync(const int32_t* tri, int64_t m, const double* s_dev,
                  const int64_t* piece_pos_dev, const int64_t* old_id_dev,
                  int64_t n_old, const int64_t* slot_pos_dev,
                  const int32_t* id_by_pos_dev, int index_dtype,
                  void* triangles_out_dev, void* triangle_source_out_dev,
                  hipStream_t s);
// Slice, the lines of one contour as records, since nothing may be written
// before every contour is counted: rec[line_pos[t]] = (t, from, to) for the
// kept lines, (from, to) = (ab, ca) with one inside, (bc, ca) with two, a
// point being its number within the contour, id_by_pos[slot_pos[e]].
int SliceLineRecordsAsync(const int32_t* tri, int64_t m, const double* s_dev,
                          double c, const int32_t* lines_dev,
                          const int64_t* line_pos_dev,
                          const int64_t* slot_pos_dev,
                          const int32_t* id_by_pos_dev, int32_t* rec_dev,
                          hipStream_t s);
// Rows line_base .. line_base + n_lines of lines_out = the records' points +
// point_base, of line_triangle_out (index dtype) their triangles, of
// line_contour_out (int32) `contour`; the last two may be NULL.
int SliceLinesOutAsync(const int32_t* rec_dev, int64_t n_lines,
                       int64_t line_base, int64_t point_base, int contour,
                       int index_dtype, void* lines_out_dev,
                       void* line_triangle_out_dev,
                       int32_t* line_contour_out_dev, hipStream_t s);

}  // namespace o3dmi
