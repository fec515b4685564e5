// Private seam between mesh_bvh.hip (a linear BVH over the triangles of one
// mesh and its closest-point query) and host/mesh_bvh.cpp (the C ABI of
// RaycastingScene::ComputeClosestPoints / ComputeDistance for one triangle
// geometry, t/geometry/RaycastingScene.cpp:206-353, 1464-1517, and of
// TriangleMesh::ComputeMetrics). Float32 only, as upstream's scene. Every
// launcher is stream-ordered and waits for nothing.
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
}
