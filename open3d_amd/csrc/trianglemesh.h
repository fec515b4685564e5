// Private seam between trianglemesh.hip (the kernels of the TriangleMesh
// operators and the two incidence structures they share) and
// host/trianglemesh.cpp (the C ABI). Every launcher is stream-ordered and
// waits for nothing; `tri` is always the triangle list as int32 {m,3} with
// every index already known to lie in [0, v) (CheckTrianglesAsync).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ransac.h"  // SplitMix64

namespace o3dmi {

constexpr int64_t kMeshMaxTriangles = 1ll << 29;  // 3 m corners < 2^31
constexpr int kMeshRun = 512;        // values added in index order per run
constexpr int kLongCornerList = 64;  // corners of a vertex one thread walks

// *bad_dev |= 1 when one of the 3 m indices lies outside [0, v); with
// narrowed_dev the indices are also written there as int32 (Int64 lists).
int CheckTrianglesAsync(const void* triangles_dev, int64_t m, int index_dtype,
                        int64_t v, int32_t* narrowed_dev, int* bad_dev,
                        hipStream_t s);

// ---- elementwise ------------------------------------------------------------
// out {m,3} = cross_3x1(p2 - p1, p3 - p1) in the position dtype.
int TriangleNormalsAsync(const void* positions_dev, int dtype,
                         const int32_t* tri, int64_t m, void* out_dev,
                         hipStream_t s);
// out {m} = 0.5 * sqrt((t0 t0 + t1 t1) + t2 t2) of that cross product.
int TriangleAreasAsync(const void* positions_dev, int dtype,
                       const int32_t* tri, int64_t m, void* out_dev,
                       hipStream_t s);
// Legacy ComputeTriangleArea in float64 from the positions widened:
// 0.5 * |(p0 - p1) x (p0 - p2)|.
int TriangleAreasF64Async(const void* positions_dev, int dtype,
                          const int32_t* tri, int64_t m, double* out_dev,
                          hipStream_t s);
// The mesh rule of NormalizeNormals, in place on {n,3}.
int NormalizeMeshNormalsAsync(void* normals_dev, int64_t n, int dtype,
                              hipStream_t s);

// The fixed float64 tree of ComputeMetrics over n >= 1 values of `dtype`:
// runs of kMeshRun values are added in index order, the run sums likewise,
// level by level; *total_dev points into sums_dev (RunSumScratchDoubles(n)
// doubles).
size_t RunSumScratchDoubles(int64_t n);
int RunSumTreeAsync(const void* values_dev, int64_t n, int dtype,
                    double* sums_dev, const double** total_dev, hipStream_t s);

// ---- uniform sampling (trianglemesh_sample.hip) --------------------------------
// The draw of point j, a pure function of (seed, j), in uint64 arithmetic
// (everything wraps): h_k = SplitMix64(seed + 0x9E3779B97F4A7C15 * (3 j + k +
// 1)) for k = 0, 1, 2 (ransac.h), and
//   u  = (double)(h_0 >> 11) * 2^-53   in [0, 1), picks the triangle,
//   r1 = (float)(h_1 >> 40) * 2^-24    in [0, 1),
//   r2 = (float)(h_2 >> 40) * 2^-24    in [0, 1).
// Both conversions and both products are exact.
struct MeshSampleDraw {
    double u;
    float r1, r2;
};
__host__ __device__ inline MeshSampleDraw DrawMeshSample(uint64_t seed,
                                                         uint64_t j) {
    const uint64_t c = 3ull * j;
    const uint64_t g = 0x9E3779B97F4A7C15ull;
    MeshSampleDraw d;
    d.u = (double)(SplitMix64(seed + g * (c + 1ull)) >> 11) *
          (1.0 / 9007199254740992.0);
    d.r1 = (float)(SplitMix64(seed + g * (c + 2ull)) >> 40) *
           (1.0f / 16777216.0f);
    d.r2 = (float)(SplitMix64(seed + g * (c + 3ull)) >> 40) *
           (1.0f / 16777216.0f);
    return d;
}

// The prefix tree of the triangle choice. Level 0 holds the m areas widened to
// double, in consecutive groups of kMeshRun: prefix[0][i] is the inclusive
// prefix of i's group, added in index order. Level k + 1 holds every group's
// last prefix of level k, grouped the same way, until a level is one group
// (m <= 2^29: at most 4 levels). The shape of RunSumTreeAsync with the
// prefixes kept; a group's prefixes are sums of non-negative values in order,
// hence monotone.
constexpr int kMeshPrefixLevels = 4;
struct MeshPrefixTree {
    int levels;
    int64_t size[kMeshPrefixLevels];
    double* prefix[kMeshPrefixLevels];
};
size_t MeshPrefixDoubles(int64_t m);
// Lays the tree out in prefix_dev (MeshPrefixDoubles(m) doubles) and fills it.
// *bad_dev |= 1 for an area that is not finite. The total area is
// tree->prefix[levels - 1][size[levels - 1] - 1].
int MeshPrefixTreeAsync(const void* areas_dev, int64_t m, int dtype,
                        double* prefix_dev, MeshPrefixTree* tree, int* bad_dev,
                        hipStream_t s);

// What a sampled point is mixed from; every pointer but positions / tri may be
// NULL. vertex_normals win over triangle_normals (both in the position dtype);
// colors are {v,3} of color_dtype O3DMI_F32 / O3DMI_U8 / O3DMI_U16.
struct MeshSampleIO {
    const void* positions;
    const int32_t* tri;
    const void* vertex_normals;
    const void* triangle_normals;
    const void* vertex_colors;
    int color_dtype;
    void* points_out;        // {n,3} position dtype
    void* normals_out;       // {n,3} position dtype
    float* colors_out;       // {n,3}
    int32_t* triangles_out;  // {n}: the triangle of every point
};
// Point j < n: x = u * total; from the top level down, in the current group
// the first i with x < prefix[i] (none, by rounding: the last i whose own
// value is > 0), x -= the prefix before i, then group i one level down. A
// triangle of area 0 is never drawn. Then TriangleMeshCPU.cpp:137-182 with
// that triangle: wts = {1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2} in
// float, out[c] = (wts[0] a[c] + wts[1] b[c]) + wts[2] c[c] (mix_3x3; a float
// times a double widens).
int MeshSamplePointsAsync(const MeshPrefixTree& tree, const void* areas_dev,
                          int dtype, const MeshSampleIO& io, int64_t n,
                          uint64_t seed, hipStream_t s);

// SamplePointsUniformly on the caller's stream for a mesh whose arguments
// were checked (host/trianglemesh.cpp): the triangle range check, the areas,
// the tree, the error downloads (one wait), then the points. io.tri is
// ignored (the checked list is used).
int SampleMeshChecked(const void* positions_dev, int64_t v, int dtype,
                      const void* triangles_dev, int64_t m, int index_dtype,
                      int64_t n, uint64_t seed, MeshSampleIO io,
                      hipStream_t s);

// ---- vertex -> corners --------------------------------------------------------
// The 3 m corner ids 3 t + k sorted stably by the vertex they name:
// corner[start[u] .. start[u] + count[u]) are the corners of vertex u in
// ascending order. vertex / corner: {3 m}; count / start: {v}.
struct CornerTable {
    uint32_t* vertex;
    uint32_t* corner;
    int32_t* count;
    int64_t* start;
};
// Bytes of scratch BuildCornerTableAsync / BuildEdgeTableAsync need (the
// sort's and the scan's, which run one after the other).
size_t IncidenceScratchBytes(int64_t m, int64_t v);
int BuildCornerTableAsync(const int32_t* tri, int64_t m, int64_t v,
                          const CornerTable& table, void* scratch_dev,
                          hipStream_t s);
// out {v,3}: component c of vertex u = ((0 + n_a[c]) + n_b[c]) + ... over u's
// corners in order, n_x the normal of the corner's triangle. One thread walks
// a list of up to kLongCornerList corners; the longer ones go to long_list
// (v + 1 ints, the last one the zeroed counter) and get a wave each.
int VertexNormalSumAsync(const CornerTable& table, int64_t v,
                         const void* triangle_normals_dev, int dtype,
                         void* out_dev, int32_t* long_list_dev, hipStream_t s);

// ---- edge -> edge slots -------------------------------------------------------
// Edge slot e = 3 t + k is the ordered pair (lo, hi) of (v_k, v_(k+1)%3). The
// table holds the 3 m slots in ascending (lo, hi, e): a run of equal (lo, hi)
// is one edge, its length the edge's multiplicity.
struct EdgeTable {
    uint32_t* lo;
    uint32_t* hi;
    uint32_t* slot;
};
__device__ __forceinline__ bool SameEdge(const EdgeTable& tb, int64_t a,
                                         int64_t b) {
    return tb.lo[a] == tb.lo[b] && tb.hi[a] == tb.hi[b];
}
// Entry j is the first one of its run.
__device__ __forceinline__ bool FirstOfRun(const EdgeTable& tb, int64_t j) {
    return j == 0 || !SameEdge(tb, j, j - 1);
}
int BuildEdgeTableAsync(const int32_t* tri, int64_t m, int64_t v,
                        const EdgeTable& table, void* scratch_dev,
                        hipStream_t s);
// flags[j] = 1 at the first slot of every edge whose multiplicity is > 2
// (allow_boundary) or != 2, else 0.
int NonManifoldFlagsAsync(const EdgeTable& table, int64_t n_slots,
                          bool allow_boundary, int32_t* flags_dev,
                          hipStream_t s);
// edges_out[pos[j]] = (lo[j], hi[j]) for the flagged slots, in the index
// dtype.
int EmitEdgesAsync(const EdgeTable& table, int64_t n_slots,
                   const int32_t* flags_dev, const int64_t* pos_dev,
                   int index_dtype, void* edges_out_dev, hipStream_t s);

// ---- connected components -----------------------------------------------------
// p[i] = i: every element its own root, the start of a union-find.
int IotaAsync(int* p_dev, int64_t n, hipStream_t s);
// root[t] = the lowest triangle index of t's component (triangles that share
// an edge of the table are adjacent), is_root[t] = (root[t] == t). parent:
// {m} ints of scratch.
int ClusterRootsAsync(const EdgeTable& table, int64_t m, int* parent_dev,
                      int* root_dev, int32_t* is_root_dev, hipStream_t s);
// labels[t] = rank[root[t]] (rank = the exclusive prefix sum of is_root), and
// counts[label] += 1 over counts zeroed by the caller.
int ClusterLabelsAsync(const int* root_dev, const int64_t* rank_dev, int64_t m,
                       int32_t* labels_dev, int32_t* counts_dev,
                       hipStream_t s);
// keys[t] = labels[t], vals[t] = t: the pairs whose stable sort lists every
// cluster's triangles in ascending index.
int LabelPairsAsync(const int32_t* labels_dev, int64_t m, uint32_t* keys_dev,
                    uint32_t* vals_dev, hipStream_t s);
// runs[c] = ceil(counts[c] / kMeshRun).
int ClusterRunCountsAsync(const int32_t* counts_dev, int64_t n_clusters,
                          int32_t* runs_dev, hipStream_t s);
// area_out[c] = the two-level sum of area[member] over the members
// sorted_tri[start[c] .. start[c] + counts[c]): run_sums[run_start[c] + r] =
// members [512 r, 512 (r + 1)) added in order, then the run sums in order.
// run_sums holds max_runs doubles (m / kMeshRun + n_clusters is enough).
int ClusterAreaSumsAsync(const double* area_dev, const uint32_t* sorted_tri_dev,
                         const int32_t* counts_dev, const int64_t* start_dev,
                         const int64_t* run_start_dev, int64_t n_clusters,
                         int64_t max_runs, double* run_sums_dev,
                         double* area_out_dev, hipStream_t s);
// out[c] = counts[c] as int64.
int WidenCountsAsync(const int32_t* counts_dev, int64_t n, int64_t* out_dev,
                     hipStream_t s);

// ---- selection ----------------------------------------------------------------
// flags[i] = (mask[i] != 0).
int MaskToFlagsAsync(const uint8_t* mask_dev, int64_t n, int32_t* flags_dev,
                     hipStream_t s);
// mask[i] = flags[i] (0 / 1).
int FlagsToMaskAsync(const int32_t* flags_dev, int64_t n, uint8_t* mask_dev,
                     hipStream_t s);
// vertex_flags[u] = 1 for every vertex of a triangle with tri_flags != 0
// (NULL: every triangle), over flags zeroed by the caller.
int MarkTriangleVerticesAsync(const int32_t* tri, int64_t m,
                              const int32_t* tri_flags_dev,
                              int32_t* vertex_flags_dev, hipStream_t s);
// vertex_flags[indices[r]] = 1 over flags zeroed by the caller; an index
// outside [0, v) is skipped and counted in *ignored_dev.
int MarkIndexedVerticesAsync(const int64_t* indices_dev, int64_t k, int64_t v,
                             int32_t* vertex_flags_dev,
                             unsigned long long* ignored_dev, hipStream_t s);
// tri_flags[t] = all three vertices of t are flagged.
int TrianglesOfVerticesAsync(const int32_t* tri, int64_t m,
                             const int32_t* vertex_flags_dev,
                             int32_t* tri_flags_dev, hipStream_t s);
// out[tri_pos[t]] = vertex_new[tri[t]] for the flagged triangles (tri_flags /
// tri_pos NULL: every triangle, in place), in the index dtype.
int RemapTrianglesAsync(const int32_t* tri, int64_t m,
                        const int32_t* tri_flags_dev,
                        const int64_t* tri_pos_dev,
                        const int64_t* vertex_new_dev, int index_dtype,
                        void* out_dev, hipStream_t s);

}  // namespace o3dmi
