// Private seam between trianglemesh_topology.hip (the kernels of the mesh
// topology and intersection queries) and host/trianglemesh_topology.cpp (the
// C ABI of legacy EulerPoincareCharacteristic, IsEdgeManifold,
// GetNonManifoldVertices, OrientTriangles, GetSelfIntersectingTriangles,
// IsIntersecting, IsWatertight and GetVolume; geometry/TriangleMesh.cpp:
// 1016-1135, 1212-1246, 1272-1457, geometry/IntersectionTest.cpp:18-56).
// Every launcher is stream-ordered and waits for nothing; `tri` is the checked
// int32 triangle list of trianglemesh.h, whose incidence tables and whose
// union-find (union_find.h) are used as they are.
//
// THE PER-PAIR FUNCTION of two triangles P = (p0, p1, p2) and Q = (q0, q1,
// q2), in float64 on the positions widened, without contraction. It is not
// symmetric: P is the lower-indexed triangle (the first mesh).
//   box(P), box(Q): the exact min / max of three doubles; they overlap by
//   IntersectionTest::AABBAABB's closed comparisons.
//   hit(P, Q): IntersectionTest::TriangleTriangle3d. mu = the six points added
//   left to right, / 6; sigma = sqrt(the six squared deviations added left to
//   right, / 5) + 1e-12 per axis; every deviation / sigma; then Moeller's
//   no-division test (JGT 2(2), 1997, as revised 1999) on the normalised
//   points, operation for operation: the six plane distances with their 1e-6
//   snap, the projection on the largest component of N1 x N2, the interval
//   test, and for coplanar triangles the projection on the largest component
//   of N1, nine edge-edge tests and two point-in-triangle tests. f64 sqrt and
//   divide are IEEE, so the result equals an SSE2 build's bit for bit.
//   The pair COUNTS iff the boxes overlap and hit.
//
// WHY THE BROAD PHASE PRUNES EXACTLY. The tree (mesh_bvh.h) holds float boxes
// of the positions narrowed with round-to-nearest. Rounding is monotone and
// so commutes with min / max: the float box of a triangle's narrowed vertices
// is the rounding of its double box, and a <= b in double implies
// round(a) <= round(b) in float. Closed overlap of two double boxes therefore
// implies closed overlap of their float boxes, and a node's box contains the
// boxes below it. A node is skipped iff its float box does not overlap the
// query triangle's float box, so no counting pair is ever skipped; at a leaf
// the exact test runs on the doubles fetched from the caller's positions,
// never on the leaf's floats. The set of counting pairs and the number of
// exact tests (pairs that pass the id and shared-vertex filters and whose
// DOUBLE boxes overlap) are pure functions of the meshes.
#pragma once

#include "common.h"
#include "mesh_bvh.h"
#include "trianglemesh.h"

namespace o3dmi {

// *count_dev (zeroed by the caller) += the sum of flags {n}.
int CountFlagsAsync(const int32_t* flags_dev, int64_t n,
                    unsigned long long* count_dev, hipStream_t s);

// ---- non-manifold vertices -------------------------------------------------------
// flags[x] = 1 iff the link edges of x's wedges (the corners of triangles that
// name x exactly once) form more than one connected component. Two wedges are
// linked iff they share a spoke (x, a), a run of the edge table: the slots of
// every run with lo != hi are united in a union-find over the 3 m corner ids,
// once by their corner at lo and once by their corner at hi (a corner of a
// triangle that names the vertex twice only ever joins that one run, so it
// connects nothing that the run does not connect already). A vertex is
// flagged iff its wedges have more than one root: a thread per corner list of
// up to kLongCornerList, a wave per longer one. parent: {3 m} ints of
// scratch; long_list: v + 1 ints, the last one the counter zeroed by the
// caller.
int NonManifoldVertexFlagsAsync(const int32_t* tri, int64_t m, int64_t v,
                                const EdgeTable& edges,
                                const CornerTable& corners, int* parent_dev,
                                int32_t* long_list_dev, int32_t* flags_dev,
                                hipStream_t s);
// out[pos[x]] = x for the flagged vertices, in the index dtype.
int EmitFlaggedAsync(const int32_t* flags_dev, const int64_t* pos_dev,
                     int64_t n, int index_dtype, void* out_dev, hipStream_t s);

// ---- orientation -------------------------------------------------------------------
// The double cover: a union-find over the 2 m nodes 2 t + s. Slot 3 t + k runs
// forward iff v_k < v_(k+1)%3; self edges are ignored. An edge of multiplicity
// > 2 sets *bad_dev; one of multiplicity 2 between two different triangles t,
// u with parity p (1: same direction) unites (2 t, 2 u + p) and (2 t + 1, 2 u
// + 1 - p). Then *bad_dev |= 1 where root(2 t) == root(2 t + 1), and flip[t] =
// root(2 t) & 1: roots are component minima, so the lowest triangle of every
// component keeps its winding. parent: {2 m} ints of scratch.
int OrientFlipsAsync(const int32_t* tri, int64_t m, const EdgeTable& edges,
                     int* parent_dev, int32_t* flip_dev, int* bad_dev,
                     hipStream_t s);
// out[t] = (a, c, b) where flip[t] and *bad_dev == 0, else (a, b, c), in the
// index dtype.
int WriteOrientedAsync(const int32_t* tri, int64_t m, const int32_t* flip_dev,
                       const int* bad_dev, int index_dtype, void* out_dev,
                       hipStream_t s);

// ---- intersections -------------------------------------------------------------------
// *bad_dev |= 1 when a coordinate of a vertex some triangle names is not
// finite, or is not finite once narrowed to float.
int CheckReferencedFiniteAsync(const void* positions_dev, int dtype,
                               const int32_t* tri, int64_t m, int* bad_dev,
                               hipStream_t s);

enum IntersectKind { kIntersectList = 0, kIntersectAny = 1 };
// The query side of a traversal. self: the queries are the tree's own
// triangles, lane by lane in sorted-leaf order, and only the pairs (i, j) with
// i < j and no shared vertex index are tested; else the queries are the m
// triangles of this (first) mesh in index order against the tree of the
// second. positions are in `dtype`, as the caller gave them.
struct IntersectQuery {
    bool self;
    const void* positions;
    int dtype;
    const int32_t* tri;
    int64_t m;
};
// What is behind the tree's leaves: the second mesh (the same one with self).
struct IntersectTarget {
    MeshBvhView bvh;
    const void* positions;
    int dtype;
    const int32_t* tri;
};
// kIntersectList: *count_dev (zeroed) += the counting pairs; the first
// `capacity` of them (in no particular order) are appended as (is_out[k],
// js_out[k]). kIntersectAny: *count_dev becomes non-zero iff a pair counts;
// every lane stops at its first pair. status_dev / visits_dev as for
// MeshBvhQueryAsync: [0] += inner nodes opened, [1] += exact pair tests.
int MeshIntersectAsync(IntersectKind kind, const IntersectQuery& query,
                       const IntersectTarget& target, uint32_t* is_out_dev,
                       uint32_t* js_out_dev, int64_t capacity,
                       unsigned long long* count_dev, int* status_dev,
                       unsigned long long* visits_dev, hipStream_t s);
// out[k] = (is[k], js[k]) in the index dtype.
int WritePairsAsync(const uint32_t* is_dev, const uint32_t* js_dev, int64_t n,
                    int index_dtype, void* out_dev, hipStream_t s);

// ---- volume ----------------------------------------------------------------------------
// out[t] = p0 . (p1 x p2) / 6 in float64 from the positions widened: every
// cross component a b - c d, the dot (x x + y y) + z z.
int TetraVolumesAsync(const void* positions_dev, int dtype, const int32_t* tri,
                      int64_t m, double* out_dev, hipStream_t s);

}  // namespace o3dmi

extern "C" {
// o3dmi_trianglemesh_get_self_intersecting_triangles (kind 0, counting only)
// or o3dmi_trianglemesh_is_self_intersecting (kind 1) with the visit counts
// ([0] inner nodes opened, [1] exact pair tests run, summed over the query
// triangles), for the bench tool and the tests. *n_out: the number of pairs
// (kind 0) or 0 / 1 (kind 1).
int o3dmi_internal_trianglemesh_self_intersections(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype, int kind,
        int64_t* n_out, unsigned long long* visits_out, o3dmi_stream_t stream);
}
