// Private seam between trianglemesh_subdivide.hip (the kernels of legacy
// SubdivideMidpoint / SubdivideLoop, geometry/TriangleMeshSubdivide.cpp) and
// host/trianglemesh_subdivide.cpp (the C ABI and the iteration driver). Every
// launcher is stream-ordered and waits for nothing; `tri` is the checked int32
// triangle list of trianglemesh.h, `table` its edge table: the 3 m edge slots
// e = 3 t + k in ascending (lo, hi, e), a run of equal (lo, hi) one edge.
//
// ONE ITERATION, index side. Upstream walks the triangles and gives the edge
// it meets first the next new vertex (:57-58, :236): the new vertex of an edge
// is v + r, r the rank of the edge's LOWEST slot among the lowest slots of all
// edges. The head of a run is that lowest slot, so a flag per slot id and its
// exclusive scan are r (EdgeSlotFlagsAsync). Edges are also numbered in table
// order, q: the inclusive scan of the head flags over the table, minus one.
// Both numberings are kept: the attribute kernels run a thread per q and write
// row v + rank[q].
#pragma once

#include "common.h"
#include "trianglemesh.h"

namespace o3dmi {

constexpr uint32_t kNoOpposite = 0xFFFFFFFFu;

// head[j] = 1 at the first entry of every run; by_slot[slot[j]] = head[j] (a
// flag per slot id: the table is a permutation of the slots, so every word is
// written once); with distinct != NULL, distinct[j] = head[j] or the entry's
// triangle differs from the one before it (the slots of one triangle are
// adjacent within a run).
int EdgeSlotFlagsAsync(const EdgeTable& table, int64_t n_slots,
                       int32_t* head_dev, int32_t* by_slot_dev,
                       int32_t* distinct_dev, hipStream_t s);

// The edges of one iteration in table order, n_edges of them. head: {n_edges +
// 1} table indices, the last one n_slots. triangles / opposite (Loop only):
// the number of distinct triangles of the edge and, per table entry, the
// vertex upstream's nested conditional (:220-225) picks in the entry's
// triangle, kNoOpposite at an entry that repeats the triangle before it.
struct SubdivEdges {
    uint32_t* lo;
    uint32_t* hi;
    int32_t* rank;
    int32_t* head;
    int32_t* triangles;
    uint32_t* opposite;
};
// The numbering chain of a table's runs, in two halves around its one wait
// (host/trianglemesh_subdivide.cpp). EdgeRunScans is what the first half
// leaves for the second: {n_slots} arrays from `tmp`, distinct / distinct_incl
// NULL unless `triangles`.
struct EdgeRunScans {
    int32_t* head;
    int32_t* distinct;
    int64_t* rank_by_slot;
    int64_t* q_incl;
    int64_t* distinct_incl;
};
// The flags, the exclusive scan of the per-slot flags into *total_dev, its
// download, with `number` the inclusive scans of head (and of distinct), then
// the wait: *n_runs_out. scratch_dev: ScanScratchBytes(n_slots).
int CountEdgeRuns(PoolScratch& tmp, const EdgeTable& table, int64_t n_slots,
                  bool number, bool triangles, void* scratch_dev,
                  long long* total_dev, EdgeRunScans* scans,
                  int64_t* n_runs_out);
// After a first half with `number`: the records of the n_runs runs from `keep`
// (triangles / opposite too when scans.distinct is there; `tri` is theirs) and
// *id_by_slot {n_slots} from `tmp`, id_base + rank of every slot's run
// (EdgeRecordsAsync, SlotVertexIdsAsync). Waits for nothing.
int NumberEdgeRuns(PoolScratch& tmp, PoolScratch& keep, const EdgeTable& table,
                   int64_t n_slots, const EdgeRunScans& scans, int64_t n_runs,
                   int64_t id_base, const int32_t* tri, SubdivEdges* edges,
                   int32_t** id_by_slot);
// Fills lo / hi / rank / head from the run heads (q = q_incl[j] - 1, rank =
// rank_by_slot[slot[j]]).
int EdgeRecordsAsync(const EdgeTable& table, int64_t n_slots,
                     const int32_t* head_dev, const int64_t* q_incl_dev,
                     const int64_t* rank_by_slot_dev, int64_t n_edges,
                     const SubdivEdges& edges, hipStream_t s);
// new_id[slot[j]] = v + rank[q_incl[j] - 1] for every table entry: the new
// vertex on each of the 3 m edge slots. With edges.opposite: that too, from
// distinct_dev and tri.
int SlotVertexIdsAsync(const EdgeTable& table, int64_t n_slots,
                       const int64_t* q_incl_dev, const SubdivEdges& edges,
                       int64_t v, const int32_t* distinct_dev,
                       const int32_t* tri, int32_t* new_id_dev, hipStream_t s);
// triangles[q] = distinct_incl[head[q + 1] - 1] - distinct_incl[head[q]] + 1.
int EdgeTriangleCountsAsync(const SubdivEdges& edges, int64_t n_edges,
                            const int64_t* distinct_incl_dev, hipStream_t s);
// Rows 4 t .. 4 t + 3 of out = (v0, v01, v20), (v01, v1, v12), (v12, v2, v20),
// (v01, v12, v20) (:77-84), in the index dtype; a thread per output word.
int EmitSubdividedAsync(const int32_t* tri, int64_t m,
                        const int32_t* new_id_dev, int index_dtype,
                        void* out_dev, hipStream_t s);

// ---- attributes: float64 {rows,3}, n_attrs of them (positions, normals,
// colours) ------------------------------------------------------------------
constexpr int kMaxSubdivAttrs = 3;
struct SubdivAttrs {
    int n_attrs;
    const double* prev[kMaxSubdivAttrs];
    double* next[kMaxSubdivAttrs];
};
// next[v + rank[q]] = 0.5 * (prev[lo] + prev[hi]) (:45-56). prev may be next:
// the rows written lie behind the rows read.
int MidpointVerticesAsync(const SubdivEdges& edges, int64_t n_edges, int64_t v,
                          const SubdivAttrs& attrs, hipStream_t s);
// long_list[long_list[n]++] = q for every run longer than kLongCornerList
// entries (n + 1 ints, the last one the counter, zeroed by the caller).
int LongEdgeRunsAsync(const SubdivEdges& edges, int64_t n_edges,
                      int32_t* long_list_dev, hipStream_t s);
// next[v + rank[q]] by :186-234: x = prev[lo] + prev[hi]; with fewer than two
// triangles x * 0.5, else x * (3. / 8.) and then += (1. / (4. * n)) *
// prev[opposite] over the run's entries in order (ascending triangle index).
// A thread per run of up to kLongCornerList entries, a wave per listed longer
// one (64 entries' rows fetched at a time, added in order).
int LoopNewVerticesAsync(const SubdivEdges& edges, int64_t n_edges, int64_t v,
                         const SubdivAttrs& attrs,
                         const int32_t* long_list_dev, hipStream_t s);
// boundary[p] = (triangles[q] == 1) at the CSR entry p of each end of every
// edge q: the place of hi in the (ascending) list of lo and of lo in the list
// of hi, by binary search. Every entry belongs to one edge and so is written.
int BoundaryFlagsAsync(const SubdivEdges& edges, int64_t n_edges,
                       const int64_t* row_splits_dev,
                       const int32_t* neighbours_dev, uint8_t* boundary_dev,
                       hipStream_t s);
// next[u] for u < v by :119-176 over u's list (BuildAdjacency's: ascending,
// without repeats): with >= 2 flagged entries beta = 1. / 8. over the flagged
// ones, else with 3 entries beta = 3. / 16., else beta = 3. / (8. * n), over
// all; alpha = 1. - count * beta; alpha * prev[u], then += beta * prev[nb] in
// list order. An empty list copies the row (upstream: NaN). A thread per list
// of up to kLongCornerList, a wave per listed longer one (long_list: v + 1
// ints, LongListsAsync).
int LoopOldVerticesAsync(const int64_t* row_splits_dev,
                         const int32_t* neighbours_dev,
                         const uint8_t* boundary_dev, int64_t v,
                         const SubdivAttrs& attrs,
                         const int32_t* long_list_dev, hipStream_t s);

}  // namespace o3dmi
