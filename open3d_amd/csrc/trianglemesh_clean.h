// Private seam between trianglemesh_clean.hip / trianglemesh_filter.hip (the
// kernels of the mesh clean-up calls, the CSR adjacency, the smoothing filters
// and the vertex clustering) and host/trianglemesh_clean.cpp /
// host/trianglemesh_filter.cpp (the C ABI). Every launcher is stream-ordered
// and waits for nothing; `tri` is the checked int32 triangle list of
// trianglemesh.h, whose incidence tables are used as they are.
#pragma once

#include "common.h"
#include "trianglemesh.h"

namespace o3dmi {

constexpr int64_t kRepMaxRows = 1ll << 30;  // int32 indices, 2 n 32-bit slots

// ---- representative table (trianglemesh_clean.hip) ----------------------------
// rep[i] = the lowest index j <= i whose key equals key i; first[i] = (rep[i]
// == i). table: RepTableSlots(n) ints (a power of two >= 2 n), filled here.
int64_t RepTableSlots(int64_t n);
// Keys: the coordinate triples by value (-0 == +0; a row with a NaN equals
// nothing: rep = i, first = 1).
int VertexRepAsync(const void* positions_dev, int64_t v, int dtype,
                   int32_t* table_dev, int64_t slots, int32_t* rep_dev,
                   int32_t* first_dev, hipStream_t s);
// Keys: int32 triples {n,3}, with `rotate` turned by RemoveDuplicatedTriangles'
// branch statements first. A row whose first word is negative is no key: rep
// = i, first = 0.
int TripleRepAsync(const int32_t* triples_dev, int64_t n, bool rotate,
                   int32_t* table_dev, int64_t slots, int32_t* rep_dev,
                   int32_t* first_dev, hipStream_t s);
// out[i] = rank[rep[i]] (rank: the exclusive prefix sum of first).
int RankOfRepAsync(const int32_t* rep_dev, const int64_t* rank_dev, int64_t n,
                   int64_t* out_dev, hipStream_t s);

// ---- triangle compaction --------------------------------------------------------
// flags[t] = t0 != t1 && t1 != t2 && t2 != t0.
int NonDegenerateFlagsAsync(const int32_t* tri, int64_t m, int32_t* flags_dev,
                            hipStream_t s);
// out[pos[t]] = row t for the flagged triangles, in the index dtype.
int CompactTrianglesAsync(const int32_t* tri, int64_t m,
                          const int32_t* flags_dev, const int64_t* pos_dev,
                          int index_dtype, void* out_dev, hipStream_t s);

// ---- CSR adjacency ----------------------------------------------------------------
// flags[j] = 1 at the first slot of every (lo, hi) run of the edge table;
// *n_self_dev (zeroed by the caller) += the runs with lo == hi.
int EdgeRunFlagsAsync(const EdgeTable& table, int64_t n_slots,
                      int32_t* flags_dev, unsigned long long* n_self_dev,
                      hipStream_t s);
// The unique edges in table order: lo_out / hi_out[pos[j]] for the flagged
// slots; upper[lo] += 1 (the neighbours >= the vertex, itself included),
// lower[hi] += 1 unless lo == hi (those below it), over counts zeroed by the
// caller.
int UniqueEdgesAsync(const EdgeTable& table, int64_t n_slots,
                     const int32_t* flags_dev, const int64_t* pos_dev,
                     uint32_t* lo_out_dev, uint32_t* hi_out_dev,
                     int32_t* upper_dev, int32_t* lower_dev, hipStream_t s);
// row_splits[u] = lower_start[u] + upper_start[u] for u < v, row_splits[v] =
// n_entries.
int AdjacencyRowsAsync(const int64_t* lower_start_dev,
                       const int64_t* upper_start_dev, int64_t v,
                       int64_t n_entries, int64_t* row_splits_dev,
                       hipStream_t s);
// Unique edge j = (lo, hi) puts hi into the list of lo behind the lower
// neighbours: slot row_splits[lo] + lower[lo] + (j - upper_start[lo]).
int AdjacencyUpperAsync(const uint32_t* lo_dev, const uint32_t* hi_dev,
                        int64_t n_edges, const int64_t* row_splits_dev,
                        const int32_t* lower_dev,
                        const int64_t* upper_start_dev, int index_dtype,
                        void* neighbours_dev, hipStream_t s);
// keys[j] = hi (v for a self edge, which sorts behind every vertex), vals[j] =
// lo: the pairs whose stable sort by key lists every vertex's lower
// neighbours in ascending order.
int ByHiPairsAsync(const uint32_t* lo_dev, const uint32_t* hi_dev,
                   int64_t n_edges, int64_t v, uint32_t* keys_dev,
                   uint32_t* vals_dev, hipStream_t s);
// Sorted pair j = (hi, lo) with hi < v puts lo into slot row_splits[hi] + (j -
// lower_start[hi]).
int AdjacencyLowerAsync(const uint32_t* keys_dev, const uint32_t* vals_dev,
                        int64_t n_edges, int64_t v,
                        const int64_t* row_splits_dev,
                        const int64_t* lower_start_dev, int index_dtype,
                        void* neighbours_dev, hipStream_t s);

// The CSR adjacency of a checked triangle list on the pool's stream
// (host/trianglemesh_clean.cpp; m, v >= 1, one wait): adj->row_splits {v + 1}
// from the pool and adj->n_entries, always. Then the lists: with `pooled` into
// adj->neighbours, an int32 array from the pool; else into neighbours_out_dev
// in the index dtype when capacity >= n_entries (capacity < 0 only counts, a
// smaller one is O3DMI_ERR_CAPACITY).
struct MeshAdjacency {
    int64_t* row_splits;
    int32_t* neighbours;
    int64_t n_entries;
};
int BuildAdjacency(PoolScratch& pool, const int32_t* tri, int64_t m, int64_t v,
                   bool pooled, int64_t capacity, int index_dtype,
                   void* neighbours_out_dev, MeshAdjacency* adj);

// ---- filters (trianglemesh_filter.hip) --------------------------------------------
constexpr int kFilterSharpen = 0, kFilterSimple = 1, kFilterLaplacian = 2;
constexpr int kMaxFilterAttrs = 3;  // positions, normals, colours

// out {n} doubles = in widened.
int WidenAsync(const void* in_dev, int64_t n, int dtype, double* out_dev,
               hipStream_t s);
// out {n} in `dtype` = in narrowed (a copy for Float64).
int NarrowAsync(const double* in_dev, int64_t n, int dtype, void* out_dev,
                hipStream_t s);
// long_list[long_list[v]++] = u for every list longer than kLongCornerList
// (v + 1 ints, the last one the counter, zeroed by the caller).
int LongListsAsync(const int64_t* row_splits_dev, int64_t v,
                   int32_t* long_list_dev, hipStream_t s);
// One pass over every vertex for the n_attrs float64 {v,3} attributes
// prev[k] -> next[k]: the statements of `kind` with `factor` (the strength /
// lambda / mu) over the vertex's list in order. The laplacian's weights come
// from ref_dev, the current positions, once per vertex for all attributes.
// Two launches: a thread per list of up to kLongCornerList, a wave per listed
// longer one (64 neighbours fetched at a time, added in order).
struct FilterPass {
    int kind;
    int n_attrs;
    const double* prev[kMaxFilterAttrs];
    double* next[kMaxFilterAttrs];
    const double* ref;
    double factor;
};
int FilterPassAsync(const int64_t* row_splits_dev,
                    const int32_t* neighbours_dev, int64_t v,
                    const FilterPass& pass, const int32_t* long_list_dev,
                    hipStream_t s);

// ---- vertex clustering (trianglemesh_clean.hip) -----------------------------------
// vox[i] = int(floor((p_i - min_bound) / voxel_size)) per axis, from the
// positions widened.
int VoxelIndicesAsync(const void* positions_dev, int64_t v, int dtype,
                      const double min_bound[3], double voxel_size,
                      int32_t* vox_dev, hipStream_t s);
// keys[i] = new_index[i], vals[i] = i, counts[new_index[i]] += 1 over counts
// zeroed by the caller.
int ClusterPairsAsync(const int64_t* new_index_dev, int64_t v,
                      uint32_t* keys_dev, uint32_t* vals_dev,
                      int32_t* counts_dev, hipStream_t s);
// plane_out {m,4} = ComputeTrianglePlane of every triangle in float64.
int TrianglePlanesAsync(const void* positions_dev, int dtype,
                        const int32_t* tri, int64_t m, double* plane_out_dev,
                        hipStream_t s);
// What a cluster is contracted from and to. members / start / counts: the
// sorted member lists. normals / colors (and their outputs) may be NULL. With
// quadric: corners (the vertex -> corners table), plane {m,4} and area {m}.
struct ClusterIO {
    const void* positions;
    const void* normals;
    const void* colors;
    const uint32_t* members;
    const int64_t* start;
    const int32_t* counts;
    bool quadric;
    CornerTable corners;
    const double* plane;
    const double* area;
    void* positions_out;
    void* normals_out;
    void* colors_out;
};
// Row c < n_clusters of every output: a thread per cluster of up to
// kLongCornerList members, a wave per longer one (long_list: n_clusters + 1
// ints, the last one the zeroed counter).
int ContractClustersAsync(const ClusterIO& io, int64_t n_clusters, int dtype,
                          int32_t* long_list_dev, hipStream_t s);
// mapped[t] = the triangle's three new indices rotated by
// SimplifyVertexClustering's statements, or (-1, -1, -1) when two are equal.
int MapClusterTrianglesAsync(const int32_t* tri, int64_t m,
                             const int64_t* new_index_dev, int32_t* mapped_dev,
                             hipStream_t s);

}  // namespace o3dmi
