// Kernels of legacy SubdivideMidpoint / SubdivideLoop (trianglemesh_subdivide.h;
// geometry/TriangleMeshSubdivide.cpp). The index side is streaming over the
// sorted edge table plus scatters by slot id; the attribute side gathers
// float64 rows (24 B) by vertex index and adds them in a fixed order, so no
// result depends on the launch geometry. Nothing here uses a float atomic, and
// the library is built without FMA contraction.
#include "trianglemesh_subdivide.h"

#include "mesh_launch.h"

namespace o3dmi {
namespace {

// ---- index side -------------------------------------------------------------------
__global__ void EdgeSlotFlagsKernel(EdgeTable tb, int64_t n3,
                                    int32_t* __restrict__ head,
                                    int32_t* __restrict__ by_slot,
                                    int32_t* __restrict__ distinct) {
    O3DMI_GRID_STRIDE(j, n3) {
        const bool first = FirstOfRun(tb, j);
        const uint32_t e = tb.slot[j];
        head[j] = first;
        by_slot[e] = first;
        if (distinct) distinct[j] = first || e / 3 != tb.slot[j - 1] / 3;
    }
}

__global__ void EdgeRecordsKernel(EdgeTable tb, int64_t n3,
                                  const int32_t* __restrict__ head,
                                  const int64_t* __restrict__ q_incl,
                                  const int64_t* __restrict__ rank_by_slot,
                                  int64_t n_edges, SubdivEdges ed) {
    O3DMI_GRID_STRIDE(j, n3 + 1) {
        if (j == n3) {
            ed.head[n_edges] = (int32_t)n3;
            continue;
        }
        if (!head[j]) continue;
        const int64_t q = q_incl[j] - 1;
        ed.lo[q] = tb.lo[j];
        ed.hi[q] = tb.hi[j];
        ed.rank[q] = (int32_t)rank_by_slot[tb.slot[j]];
        ed.head[q] = (int32_t)j;
    }
}

__global__ void SlotVertexIdsKernel(EdgeTable tb, int64_t n3,
                                    const int64_t* __restrict__ q_incl,
                                    SubdivEdges ed, int64_t v,
                                    const int32_t* __restrict__ distinct,
                                    const int32_t* __restrict__ tri,
                                    int32_t* __restrict__ new_id) {
    O3DMI_GRID_STRIDE(j, n3) {
        const uint32_t e = tb.slot[j];
        new_id[e] = (int32_t)(v + ed.rank[q_incl[j] - 1]);
        if (!ed.opposite) continue;
        uint32_t opp = kNoOpposite;
        if (distinct[j]) {
            const uint32_t a = tb.lo[j], b = tb.hi[j];
            const int32_t* row = tri + 3 * (int64_t)(e / 3);
            const uint32_t t0 = row[0], t1 = row[1], t2 = row[2];
            opp = (t0 != a && t0 != b) ? t0
                                       : ((t1 != a && t1 != b) ? t1 : t2);
        }
        ed.opposite[j] = opp;
    }
}

__global__ void EdgeTriangleCountsKernel(SubdivEdges ed, int64_t n_edges,
                                         const int64_t* __restrict__ incl) {
    O3DMI_GRID_STRIDE(q, n_edges)
        ed.triangles[q] =
                (int32_t)(incl[ed.head[q + 1] - 1] - incl[ed.head[q]] + 1);
}

// Word c of a triangle's 12 output words: 0..2 its own corners, 3..5 the new
// vertices of its slots 0 (v01), 1 (v12), 2 (v20); a nibble per word.
constexpr unsigned long long kEmitSources = 0x543524413530ull;

template <typename I>
__global__ void EmitSubdividedKernel(const int32_t* __restrict__ tri,
                                     int64_t m,
                                     const int32_t* __restrict__ new_id,
                                     I* __restrict__ out) {
    O3DMI_GRID_STRIDE(i, 12 * m) {
        const int64_t t = i / 12;
        const int c = (int)(i - 12 * t);
        const int src = (int)((kEmitSources >> (4 * c)) & 7);
        out[i] = (I)(src < 3 ? tri[3 * t + src] : new_id[3 * t + src - 3]);
    }
}

// ---- attributes -------------------------------------------------------------------
template <int kAttrs>
__global__ void MidpointVerticesKernel(SubdivEdges ed, int64_t n_edges,
                                       int64_t v, SubdivAttrs at) {
    O3DMI_GRID_STRIDE(q, n_edges) {
        const int64_t a = ed.lo[q], b = ed.hi[q], row = v + ed.rank[q];
#pragma unroll
        for (int k = 0; k < kAttrs; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                at.next[k][3 * row + c] =
                        0.5 * (at.prev[k][3 * a + c] + at.prev[k][3 * b + c]);
    }
}

__global__ void LongEdgeRunsKernel(SubdivEdges ed, int64_t n_edges,
                                   int32_t* __restrict__ long_list) {
    O3DMI_GRID_STRIDE(q, n_edges)
        if (ed.head[q + 1] - ed.head[q] > kLongCornerList)
            long_list[atomicAdd(&long_list[n_edges], 1)] = (int32_t)q;
}

// :186-215: the two ends added, then scaled by the edge's weight.
template <int kAttrs>
__device__ __forceinline__ void LoopEdgeEnds(const SubdivEdges& ed,
                                             const SubdivAttrs& at, int64_t q,
                                             int n, double x[kAttrs][3]) {
    const int64_t a = ed.lo[q], b = ed.hi[q];
    const double w = n < 2 ? 0.5 : 3. / 8.;
#pragma unroll
    for (int k = 0; k < kAttrs; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            x[k][c] = (at.prev[k][3 * a + c] + at.prev[k][3 * b + c]) * w;
}

template <int kAttrs>
__device__ __forceinline__ void StoreRow(const SubdivAttrs& at, int64_t row,
                                         const double x[kAttrs][3]) {
#pragma unroll
    for (int k = 0; k < kAttrs; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) at.next[k][3 * row + c] = x[k][c];
}

template <int kAttrs>
__global__ void LoopNewThreadKernel(SubdivEdges ed, int64_t n_edges, int64_t v,
                                    SubdivAttrs at) {
    O3DMI_GRID_STRIDE(q, n_edges) {
        const int begin = ed.head[q], cnt = ed.head[q + 1] - begin;
        if (cnt > kLongCornerList) continue;  // LoopNewWaveKernel's
        const int n = ed.triangles[q];
        double x[kAttrs][3];
        LoopEdgeEnds<kAttrs>(ed, at, q, n, x);
        if (n >= 2) {
            const double scale = 1. / (4. * (double)n);
            for (int j = 0; j < cnt; ++j) {
                const uint32_t o = ed.opposite[begin + j];
                if (o == kNoOpposite) continue;
#pragma unroll
                for (int k = 0; k < kAttrs; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        x[k][c] += scale * at.prev[k][3 * (int64_t)o + c];
            }
        }
        StoreRow<kAttrs>(at, v + ed.rank[q], x);
    }
}

// A wave per listed run: 64 entries' opposite rows are fetched and scaled at
// once, then added in entry order (every lane does the same adds; lane 0
// stores). A run this long has n >= 2: at most three entries name a triangle.
template <int kAttrs>
__global__ void LoopNewWaveKernel(SubdivEdges ed, int64_t n_edges, int64_t v,
                                  SubdivAttrs at,
                                  const int32_t* __restrict__ long_list) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int n_long = long_list[n_edges];
    for (int64_t w = wave; w < n_long; w += n_waves) {
        const int64_t q = long_list[w];
        const int begin = ed.head[q], cnt = ed.head[q + 1] - begin;
        const int n = ed.triangles[q];
        double x[kAttrs][3];
        LoopEdgeEnds<kAttrs>(ed, at, q, n, x);
        const double scale = 1. / (4. * (double)n);
        for (int j0 = 0; n >= 2 && j0 < cnt; j0 += 64) {
            double p[kAttrs][3];
#pragma unroll
            for (int k = 0; k < kAttrs; ++k) p[k][0] = p[k][1] = p[k][2] = 0.0;
            uint32_t o = kNoOpposite;
            if (j0 + lane < cnt) o = ed.opposite[begin + j0 + lane];
            if (o != kNoOpposite) {
#pragma unroll
                for (int k = 0; k < kAttrs; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        p[k][c] = scale * at.prev[k][3 * (int64_t)o + c];
            }
            const unsigned long long use = __ballot(o != kNoOpposite);
            const int len = cnt - j0 < 64 ? cnt - j0 : 64;
            for (int l = 0; l < len; ++l) {
                if (!((use >> l) & 1)) continue;  // wave-uniform
#pragma unroll
                for (int k = 0; k < kAttrs; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) x[k][c] += __shfl(p[k][c], l);
            }
        }
        if (lane == 0) StoreRow<kAttrs>(at, v + ed.rank[q], x);
    }
}

// The first place >= target in the ascending list [begin, end).
__device__ __forceinline__ int64_t LowerBound(const int32_t* list,
                                              int64_t begin, int64_t end,
                                              int32_t target) {
    while (begin < end) {
        const int64_t mid = begin + ((end - begin) >> 1);
        if (list[mid] < target) begin = mid + 1;
        else end = mid;
    }
    return begin;
}

__global__ void BoundaryFlagsKernel(SubdivEdges ed, int64_t n_edges,
                                    const int64_t* __restrict__ row_splits,
                                    const int32_t* __restrict__ neighbours,
                                    uint8_t* __restrict__ boundary) {
    O3DMI_GRID_STRIDE(q, n_edges) {
        const int32_t a = (int32_t)ed.lo[q], b = (int32_t)ed.hi[q];
        const uint8_t flag = ed.triangles[q] == 1;
        const int64_t end_a = row_splits[a + 1];
        const int64_t pa = LowerBound(neighbours, row_splits[a], end_a, b);
        if (pa < end_a && neighbours[pa] == b) boundary[pa] = flag;
        if (a == b) continue;
        const int64_t end_b = row_splits[b + 1];
        const int64_t pb = LowerBound(neighbours, row_splits[b], end_b, a);
        if (pb < end_b && neighbours[pb] == a) boundary[pb] = flag;
    }
}

// :135-145 for a list of cnt entries, n_boundary of them flagged; returns
// whether only the flagged ones are added.
__device__ __forceinline__ bool LoopVertexWeights(int cnt, int n_boundary,
                                                  double* alpha,
                                                  double* beta) {
    if (n_boundary >= 2) {
        *beta = 1. / 8.;
        *alpha = 1. - (double)n_boundary * *beta;
        return true;
    }
    if (cnt == 3) {
        *beta = 3. / 16.;
    } else {
        *beta = 3. / (8. * (double)cnt);
    }
    *alpha = 1. - (double)cnt * *beta;
    return false;
}

template <int kAttrs>
__global__ void LoopOldThreadKernel(const int64_t* __restrict__ row_splits,
                                    const int32_t* __restrict__ neighbours,
                                    const uint8_t* __restrict__ boundary,
                                    int64_t v, SubdivAttrs at) {
    O3DMI_GRID_STRIDE(u, v) {
        const int64_t begin = row_splits[u];
        const int64_t size = row_splits[u + 1] - begin;
        if (size > kLongCornerList) continue;  // LoopOldWaveKernel's
        const int cnt = (int)size;
        double x[kAttrs][3];
#pragma unroll
        for (int k = 0; k < kAttrs; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) x[k][c] = at.prev[k][3 * u + c];
        if (cnt > 0) {
            int n_boundary = 0;
            for (int j = 0; j < cnt; ++j) n_boundary += boundary[begin + j];
            double alpha, beta;
            const bool flagged_only =
                    LoopVertexWeights(cnt, n_boundary, &alpha, &beta);
#pragma unroll
            for (int k = 0; k < kAttrs; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) x[k][c] = alpha * x[k][c];
            for (int j = 0; j < cnt; ++j) {
                if (flagged_only && !boundary[begin + j]) continue;
                const int64_t i = neighbours[begin + j];
#pragma unroll
                for (int k = 0; k < kAttrs; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        x[k][c] += beta * at.prev[k][3 * i + c];
            }
        }
        StoreRow<kAttrs>(at, u, x);
    }
}

template <int kAttrs>
__global__ void LoopOldWaveKernel(const int64_t* __restrict__ row_splits,
                                  const int32_t* __restrict__ neighbours,
                                  const uint8_t* __restrict__ boundary,
                                  int64_t v, SubdivAttrs at,
                                  const int32_t* __restrict__ long_list) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int n_long = long_list[v];
    for (int64_t w = wave; w < n_long; w += n_waves) {
        const int64_t u = long_list[w];
        const int64_t begin = row_splits[u];
        const int cnt = (int)(row_splits[u + 1] - begin);
        int n_boundary = 0;
        for (int j0 = 0; j0 < cnt; j0 += 64)
            n_boundary += __popcll(
                    __ballot(j0 + lane < cnt && boundary[begin + j0 + lane]));
        double alpha, beta;
        const bool flagged_only =
                LoopVertexWeights(cnt, n_boundary, &alpha, &beta);
        double x[kAttrs][3];
#pragma unroll
        for (int k = 0; k < kAttrs; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                x[k][c] = alpha * at.prev[k][3 * u + c];
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            double p[kAttrs][3];
#pragma unroll
            for (int k = 0; k < kAttrs; ++k) p[k][0] = p[k][1] = p[k][2] = 0.0;
            const bool mine = j0 + lane < cnt &&
                              (!flagged_only || boundary[begin + j0 + lane]);
            if (mine) {
                const int64_t i = neighbours[begin + j0 + lane];
#pragma unroll
                for (int k = 0; k < kAttrs; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        p[k][c] = beta * at.prev[k][3 * i + c];
            }
            const unsigned long long use = __ballot(mine);
            const int len = cnt - j0 < 64 ? cnt - j0 : 64;
            for (int l = 0; l < len; ++l) {
                if (!((use >> l) & 1)) continue;  // wave-uniform
#pragma unroll
                for (int k = 0; k < kAttrs; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) x[k][c] += __shfl(p[k][c], l);
            }
        }
        if (lane == 0) StoreRow<kAttrs>(at, u, x);
    }
}

int CheckAttrs(const SubdivAttrs& attrs) {
    O3DMI_REQUIRE(attrs.n_attrs >= 1 && attrs.n_attrs <= kMaxSubdivAttrs,
                  "subdivide: 1 to 3 attributes");
    return O3DMI_OK;
}

}  // namespace

int EdgeSlotFlagsAsync(const EdgeTable& table, int64_t n_slots,
                       int32_t* head_dev, int32_t* by_slot_dev,
                       int32_t* distinct_dev, hipStream_t s) {
    O3DMI_LAUNCH(EdgeSlotFlagsKernel, n_slots, table, n_slots, head_dev,
                 by_slot_dev, distinct_dev);
    return O3DMI_OK;
}

int EdgeRecordsAsync(const EdgeTable& table, int64_t n_slots,
                     const int32_t* head_dev, const int64_t* q_incl_dev,
                     const int64_t* rank_by_slot_dev, int64_t n_edges,
                     const SubdivEdges& edges, hipStream_t s) {
    O3DMI_LAUNCH(EdgeRecordsKernel, n_slots + 1, table, n_slots, head_dev,
                 q_incl_dev, rank_by_slot_dev, n_edges, edges);
    return O3DMI_OK;
}

int SlotVertexIdsAsync(const EdgeTable& table, int64_t n_slots,
                       const int64_t* q_incl_dev, const SubdivEdges& edges,
                       int64_t v, const int32_t* distinct_dev,
                       const int32_t* tri, int32_t* new_id_dev,
                       hipStream_t s) {
    O3DMI_REQUIRE(!edges.opposite || (distinct_dev && tri), "null argument");
    O3DMI_LAUNCH(SlotVertexIdsKernel, n_slots, table, n_slots, q_incl_dev,
                 edges, v, distinct_dev, tri, new_id_dev);
    return O3DMI_OK;
}

int EdgeTriangleCountsAsync(const SubdivEdges& edges, int64_t n_edges,
                            const int64_t* distinct_incl_dev, hipStream_t s) {
    O3DMI_LAUNCH(EdgeTriangleCountsKernel, n_edges, edges, n_edges,
                 distinct_incl_dev);
    return O3DMI_OK;
}

int EmitSubdividedAsync(const int32_t* tri, int64_t m,
                        const int32_t* new_id_dev, int index_dtype,
                        void* out_dev, hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(EmitSubdividedKernel<int64_t>, 12 * m, tri, m, new_id_dev,
                     (int64_t*)out_dev);
    else
        O3DMI_LAUNCH(EmitSubdividedKernel<int32_t>, 12 * m, tri, m, new_id_dev,
                     (int32_t*)out_dev);
    return O3DMI_OK;
}

int MidpointVerticesAsync(const SubdivEdges& edges, int64_t n_edges, int64_t v,
                          const SubdivAttrs& attrs, hipStream_t s) {
    const int st = CheckAttrs(attrs);
    if (st) return st;
    switch (attrs.n_attrs) {
        case 1:
            O3DMI_LAUNCH(MidpointVerticesKernel<1>, n_edges, edges, n_edges, v,
                         attrs);
            break;
        case 2:
            O3DMI_LAUNCH(MidpointVerticesKernel<2>, n_edges, edges, n_edges, v,
                         attrs);
            break;
        default:
            O3DMI_LAUNCH(MidpointVerticesKernel<3>, n_edges, edges, n_edges, v,
                         attrs);
    }
    return O3DMI_OK;
}

int LongEdgeRunsAsync(const SubdivEdges& edges, int64_t n_edges,
                      int32_t* long_list_dev, hipStream_t s) {
    O3DMI_LAUNCH(LongEdgeRunsKernel, n_edges, edges, n_edges, long_list_dev);
    return O3DMI_OK;
}

namespace {

template <int kAttrs>
int LaunchLoopNew(const SubdivEdges& edges, int64_t n_edges, int64_t v,
                  const SubdivAttrs& attrs, const int32_t* long_list_dev,
                  hipStream_t s) {
    O3DMI_LAUNCH(LoopNewThreadKernel<kAttrs>, n_edges, edges, n_edges, v,
                 attrs);
    hipLaunchKernelGGL(LoopNewWaveKernel<kAttrs>, WaveGrid(n_edges),
                       dim3(kBlock), 0, s, edges, n_edges, v, attrs,
                       long_list_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

template <int kAttrs>
int LaunchLoopOld(const int64_t* row_splits_dev, const int32_t* neighbours_dev,
                  const uint8_t* boundary_dev, int64_t v,
                  const SubdivAttrs& attrs, const int32_t* long_list_dev,
                  hipStream_t s) {
    O3DMI_LAUNCH(LoopOldThreadKernel<kAttrs>, v, row_splits_dev,
                 neighbours_dev, boundary_dev, v, attrs);
    hipLaunchKernelGGL(LoopOldWaveKernel<kAttrs>, WaveGrid(v), dim3(kBlock), 0,
                       s, row_splits_dev, neighbours_dev, boundary_dev, v,
                       attrs, long_list_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace

int LoopNewVerticesAsync(const SubdivEdges& edges, int64_t n_edges, int64_t v,
                         const SubdivAttrs& attrs,
                         const int32_t* long_list_dev, hipStream_t s) {
    const int st = CheckAttrs(attrs);
    if (st) return st;
    switch (attrs.n_attrs) {
        case 1:
            return LaunchLoopNew<1>(edges, n_edges, v, attrs, long_list_dev, s);
        case 2:
            return LaunchLoopNew<2>(edges, n_edges, v, attrs, long_list_dev, s);
        default:
            return LaunchLoopNew<3>(edges, n_edges, v, attrs, long_list_dev, s);
    }
}

int BoundaryFlagsAsync(const SubdivEdges& edges, int64_t n_edges,
                       const int64_t* row_splits_dev,
                       const int32_t* neighbours_dev, uint8_t* boundary_dev,
                       hipStream_t s) {
    O3DMI_LAUNCH(BoundaryFlagsKernel, n_edges, edges, n_edges, row_splits_dev,
                 neighbours_dev, boundary_dev);
    return O3DMI_OK;
}

int LoopOldVerticesAsync(const int64_t* row_splits_dev,
                         const int32_t* neighbours_dev,
                         const uint8_t* boundary_dev, int64_t v,
                         const SubdivAttrs& attrs,
                         const int32_t* long_list_dev, hipStream_t s) {
    const int st = CheckAttrs(attrs);
    if (st) return st;
    switch (attrs.n_attrs) {
        case 1:
            return LaunchLoopOld<1>(row_splits_dev, neighbours_dev,
                                    boundary_dev, v, attrs, long_list_dev, s);
        case 2:
            return LaunchLoopOld<2>(row_splits_dev, neighbours_dev,
                                    boundary_dev, v, attrs, long_list_dev, s);
        default:
            return LaunchLoopOld<3>(row_splits_dev, neighbours_dev,
                                    boundary_dev, v, attrs, long_list_dev, s);
    }
}

}  // namespace o3dmi
