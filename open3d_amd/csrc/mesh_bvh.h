// Private seam between mesh_bvh.hip (a linear BVH over the triangles of one
// mesh, its closest-point query and its ray queries) and host/mesh_bvh.cpp
// (the C ABI of RaycastingScene::ComputeClosestPoints / ComputeDistance for
// one triangle geometry, t/geometry/RaycastingScene.cpp:206-353, 1464-1517,
// of TriangleMesh::ComputeMetrics, and of CastRays, TestOcclusions,
// CountIntersections, ListIntersections, ComputeOccupancy,
// ComputeSignedDistance and CreateRaysPinhole, :486-1100, 1325-1462,
// 1520-1674). Float32 only, as upstream's scene. Every launcher is
// stream-ordered and waits for nothing.
//
// THE PER-PAIR FUNCTION. For a query q and a triangle t = (a, b, c), in float
// without contraction, every dot product (x x + y y) + z z:
//   p, u, v = upstream's closestPointTriangle, branch for branch;
//   e2 = ((dx dx) + dy dy) + dz dz of q - p;
//   b2 = the same expression on the per-axis gap between q and t's own
//        bounding box, max(lo - q, q - hi, 0) (the box is exact: a min / max
//        of three floats);
//   d2(q, t) = max(e2, b2).
// A NaN e2 (a degenerate triangle makes 0 / 0 in the edge branches) stays NaN
// and never wins, as upstream's `d < radius` never accepts it.
//
// Why the max: closestPointTriangle has no usable error bound on slivers (va,
// vb, vc cancel), so its e2 can come out below what any bounding box allows,
// and a tree that prunes on box distances would then answer differently from
// an exhaustive loop. With the clamp pruning is exact: float subtract,
// multiply, add and max are monotone, so the b2 expression on a node's box
// (which contains the boxes below it) is <= the d2 of every triangle under
// the node. The clamp changes e2 only where e2 is already a rounding
// artefact.
//
// THE RESULT of a query is the minimum of d2(q, t) over all triangles; on
// equal d2 the lowest triangle index wins (a node is skipped only when its
// bound is > the best, strictly). It is a pure function of the mesh and the
// query: the same for any tree, traversal order and launch shape. When no
// triangle has a non-NaN d2: id 0xFFFFFFFF, distance +inf, the other rows 0.
//
// THE PER-PAIR FUNCTION OF A RAY. A ray is (o, d) with a range (tnear, tfar];
// d is not normalised and t is in units of |d|. For a triangle t = (a, b, c),
// in float without contraction, every dot product (x x + y y) + z z, every
// cross product's component x y - z w:
//   e1 = b - a, e2 = c - a, p = d x e2, det = e1 . p;
//   a miss when det == 0 or det is NaN (a degenerate triangle and a zero
//   direction never hit); no back-face culling;
//   inv = 1 / det, s = o - a, u = (s . p) inv, q = s x e1, v = (d . q) inv,
//   t_e = (e2 . q) inv;  hit_e = u >= 0 && v >= 0 && u + v <= 1
//   (Moeller-Trumbore; u weighs b and v weighs c, as the closest point's uvs);
//   the slab interval [T0, T1] of a box [lo, hi]: per axis with d_k != 0,
//   t1 = (lo_k - o_k) / d_k, t2 = (hi_k - o_k) / d_k (a division, never a
//   reciprocal), enter_k = min, exit_k = max; per axis with d_k == 0 the
//   interval is empty when o_k < lo_k || o_k > hi_k and otherwise unbounded;
//   T0 = max(enter_x, enter_y, enter_z, tnear), T1 = min(exit_x, exit_y,
//   exit_z, tfar); non-empty iff T0 <= T1;
//   with [T0, T1] taken on t's OWN bounding box (exact, as above):
//   the pair hits iff hit_e && T0 <= T1 && t_e > tnear && t_e <= tfar, and
//   its parameter is t = min(max(t_e, T0), T1) + 0 (the + 0 makes a zero
//   positive: the sign of a zero T0 depends on which of two equal operands a
//   min returns).
//
// Why the clamp: with finite input a float subtract and a divide by a fixed
// non-zero d_k produce no NaN and are monotone, and so are min and max. The
// interval of any box that contains t's box therefore contains t's [T0, T1],
// hence the pair's parameter. A node can be skipped exactly when its interval
// is empty or its T0 is > the best t (strictly: a node at the best t may hold
// a lower index). The clamp moves t_e only where it already disagrees with
// the triangle's own box, that is, where it is a rounding artefact.
//
// THE RESULTS OF THE RAY QUERIES, pure functions of the mesh and the ray:
//   closest  the minimum t over the hitting pairs, the lowest triangle index
//            on equal t; u, v recomputed from the winner; no hit: t = +inf,
//            ids 0xFFFFFFFF, the other rows 0;
//   any      whether a hitting pair exists;
//   count    the number of DISTINCT values of t among the hitting pairs
//            (tnear = 0, tfar = +inf), found by iterating "the smallest t
//            strictly above the previous one" (a node is also skipped when
//            its T1 is <= the previous t);
//   list     one entry per distinct t in ascending order, the lowest triangle
//            index at that t;
//   vote     a point is inside when more than nsamples / 2 of its rays
//            (o3dmi_raycast_vote_directions) have an odd count.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "o3d_mi355x.h"

namespace o3dmi {

constexpr int kBvhMortonBits = 30;  // 10 per axis
// The stack of a query. A push happens once per level of the path, and the
// radix tree over the keys (code, sorted position) is no deeper than the
// number of key bits that can differ, 30 + BitsFor(m) <= 59 for m <= 2^29.
constexpr int kBvhStack = 64;
constexpr uint32_t kBvhNoTriangle = 0xFFFFFFFFu;

// An inner node: its two children with their boxes. child >= 0 is an inner
// node, child < 0 the leaf ~child (a sorted position). 64 bytes.
struct alignas(16) BvhNode {
    int32_t child[2];
    int32_t parent;    // (parent node << 1) | side, -1 for the root
    int32_t arrivals;  // the refit's counter
    float box[2][6];   // lo xyz, hi xyz of either child
};
// A leaf: one triangle, its vertices gathered. 48 bytes.
struct alignas(16) BvhLeaf {
    float a[3], b[3], c[3];
    uint32_t id;      // the triangle's index in the mesh
    int32_t parent;   // as BvhNode::parent
    uint32_t pad;
};

struct MeshBvhView {
    const BvhNode* nodes;  // m - 1
    const BvhLeaf* leaves; // m, in sorted order
    int64_t m;
    float scene_lo[3], scene_hi[3];
};

// Bytes of scratch BuildMeshBvhAsync needs besides nodes and leaves.
size_t MeshBvhBuildScratchBytes(int64_t m);
// Builds nodes {m - 1} and leaves {m} from checked int32 triangles and finite
// positions. scene_dev: 6 floats, the box of the referenced vertices.
int BuildMeshBvhAsync(const float* positions_dev, const int32_t* tri,
                      int64_t m, BvhNode* nodes_dev, BvhLeaf* leaves_dev,
                      float* scene_dev, void* scratch_dev, hipStream_t s);

// The optional outputs of a query, RaycastingScene::ComputeClosestPoints'.
struct MeshQueryOut {
    float* points;       // {q,3}
    uint32_t* ids;       // {q}
    float* uvs;          // {q,2}
    float* normals;      // {q,3}
    float* distance;     // {q} sqrt(d2)
    float* d2;           // {q}
};
// Bytes of scratch a query with sort_queries needs (0 without).
size_t MeshBvhQueryScratchBytes(int64_t q);
// status_dev (zeroed by the caller): |= 1 when a stack would have overflowed
// (the results are then not to be used). visits_dev (optional, zeroed): [0] +=
// inner nodes opened, [1] += triangles tested. sort_queries: lanes take the
// queries in the order of their Morton codes in the scene box; the outputs
// are in input order with the same bits either way.
int MeshBvhQueryAsync(const MeshBvhView& bvh, const float* queries_dev,
                      int64_t q, const MeshQueryOut& out, bool sort_queries,
                      void* scratch_dev, int* status_dev,
                      unsigned long long* visits_dev, hipStream_t s);

// ---- ray queries (the second comment block at the top) --------------------------
enum RayQueryKind { kRayClosest = 0, kRayAny = 1, kRayCount = 2 };
// What a ray query writes; every pointer is optional. kRayClosest: t_hit {q},
// geometry_ids {q} (0 on a hit), primitive_ids {q}, uvs {q,2}, normals {q,3}
// (the closest point's mesh rule). kRayAny: occluded {q} 0 / 1. kRayCount:
// counts {q}.
struct RayQueryOut {
    float* t_hit;
    uint32_t* geometry_ids;
    uint32_t* primitive_ids;
    float* uvs;
    float* normals;
    uint8_t* occluded;
    int32_t* counts;
};
// rays_dev {q,6} finite; tnear / tfar not NaN (kRayCount takes 0 and +inf).
// scratch_dev, status_dev, visits_dev and sort_rays (by the Morton code of
// the origin) as for MeshBvhQueryAsync, MeshBvhQueryScratchBytes(q) included.
int MeshBvhRayQueryAsync(const MeshBvhView& bvh, RayQueryKind kind,
                         const float* rays_dev, int64_t q, float tnear,
                         float tfar, const RayQueryOut& out, bool sort_rays,
                         void* scratch_dev, int* status_dev,
                         unsigned long long* visits_dev, hipStream_t s);

// The entries of the list query, each optional, written at splits_dev[ray] +
// k for the k-th distinct t of the ray in ascending order.
struct RayListOut {
    int64_t* ray_ids;
    float* t_hit;
    uint32_t* geometry_ids;
    uint32_t* primitive_ids;
    float* uvs;  // {total,2}
};
// splits_dev {q}: the exclusive prefix sum of the kRayCount counts.
int MeshBvhRayListAsync(const MeshBvhView& bvh, const float* rays_dev,
                        int64_t q, const int64_t* splits_dev,
                        const RayListOut& out, int* status_dev, hipStream_t s);

// The inside / outside vote of points_dev {q,3} (finite) over the rays
// (point, dirs_dev[j]), j < nsamples, in up to eight neighbouring lanes of
// one wave: no ray or count tensor exists.
// occupancy_out_dev {q} (optional): 1 inside, 0 outside. distance_io_dev {q}
// (optional): multiplied by -1 inside and by +1 outside.
int MeshBvhVoteAsync(const MeshBvhView& bvh, const float* points_dev,
                     int64_t q, const float* dirs_dev, int nsamples,
                     float* occupancy_out_dev, float* distance_io_dev,
                     int* status_dev, hipStream_t s);

// The host half of CreateRaysPinhole, narrowed once: the camera centre and
// R^T K^-1, row-major.
struct PinholeFrame {
    float centre[3];
    float dir[9];
};
// rays_out_dev {height, width, 6}: the centre and dir (x + 0.5, y + 0.5, 1),
// every row (m0 px + m1 py) + m2.
int CreateRaysPinholeAsync(const PinholeFrame& frame, int width, int height,
                           float* rays_out_dev, hipStream_t s);

}  // namespace o3dmi

// The C struct behind o3dmi_mesh_bvh_t: the handle owns its copies.
struct o3dmi_mesh_bvh {
    o3dmi::BvhNode* nodes = nullptr;
    o3dmi::BvhLeaf* leaves = nullptr;
    int64_t m = 0;
    float scene[6] = {0, 0, 0, 0, 0, 0};
};

extern "C" {
// o3dmi_mesh_bvh_closest_points with the query order chosen by the caller and
// the visit counts ([0] inner nodes opened, [1] triangles tested, summed over
// the queries; NULL: not wanted), for the bench tool and the tests.
int o3dmi_internal_mesh_bvh_query(const struct o3dmi_mesh_bvh* bvh,
                                  const void* queries_dev, int64_t q,
                                  void* points_out_dev,
                                  uint32_t* primitive_ids_out_dev,
                                  void* primitive_uvs_out_dev,
                                  void* primitive_normals_out_dev,
                                  void* distance_out_dev, int sort_queries,
                                  unsigned long long* visits_out,
                                  o3dmi_stream_t stream);
// o3dmi_mesh_bvh_cast_rays (kind 0: t_hit, geometry_ids, primitive_ids, uvs,
// normals), _test_occlusions (kind 1: occluded) or _count_intersections (kind
// 2: counts; tnear and tfar are ignored) with the ray order chosen by the
// caller and the visit counts, as above.
int o3dmi_internal_mesh_bvh_ray_query(
        const struct o3dmi_mesh_bvh* bvh, int kind, const void* rays_dev,
        int64_t q, float tnear, float tfar, void* t_hit_out_dev,
        uint32_t* geometry_ids_out_dev, uint32_t* primitive_ids_out_dev,
        void* primitive_uvs_out_dev, void* primitive_normals_out_dev,
        uint8_t* occluded_out_dev, int32_t* counts_out_dev, int sort_rays,
        unsigned long long* visits_out, o3dmi_stream_t stream);
}
