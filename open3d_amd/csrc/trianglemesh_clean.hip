// Kernels of the mesh clean-up calls, the CSR adjacency and the vertex
// clustering (trianglemesh_clean.h): legacy geometry/TriangleMesh.cpp:153-165
// and 680-860 and TriangleMeshSimplification.cpp:72-244 on the device.
//
//   representative table   the open-addressing table of row INDICES of
//       rep_table.h (RemoveDuplicatedPoints' table) with three ways of making
//       a row a key of three words: equal keys meet in one slot and keep the
//       lowest index with atomicMin, so rep[] is a pure function of the
//       input. One insert and one look-up launch; a probe is one atomic or one
//       load plus the resident row's key (load factor <= 1/2).
//   adjacency              the unique (lo, hi) runs of the edge table put hi
//       into the list of lo directly (the table is sorted by (lo, hi)); one
//       more stable sort by hi puts lo into the list of hi. No search.
//   clustering             member lists from the pair sort of (new index, old
//       index); a thread walks a list in order, a wave a long one.
//
// No float is added in arrival order: the only atomics are integer counts,
// the table's CAS / min and the long-list counters.
#include "trianglemesh_clean.h"

#include "mesh_launch.h"
#include "rep_table.h"
#include "scan.h"
#include "sort.h"

namespace o3dmi {
namespace {

// ---- representative table ---------------------------------------------------------
__device__ __forceinline__ uint32_t BitsOf(float x) {
    return __float_as_uint(x);
}
__device__ __forceinline__ uint64_t BitsOf(double x) {
    return (uint64_t)__double_as_longlong(x);
}

// The coordinates by value: both zeros are one word, every other value that
// is no NaN has one bit pattern.
template <typename T, typename W>
struct VertexKeys {
    using Word = W;
    const T* p;
    __device__ __forceinline__ int operator()(int64_t i, W k[3]) const {
        const T x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        if (x != x || y != y || z != z) return kAlone;
        k[0] = BitsOf(x == 0 ? (T)0 : x);
        k[1] = BitsOf(y == 0 ? (T)0 : y);
        k[2] = BitsOf(z == 0 ? (T)0 : z);
        return kKeyed;
    }
};

struct TripleKeys {
    using Word = uint32_t;
    const int32_t* t;
    bool rotate;
    __device__ __forceinline__ int operator()(int64_t i, uint32_t k[3]) const {
        const int32_t a = t[3 * i], b = t[3 * i + 1], c = t[3 * i + 2];
        if (a < 0) return kNoKey;
        int32_t r0 = a, r1 = b, r2 = c;
        if (rotate) {  // geometry/TriangleMesh.cpp:744-760
            if (a <= b) {
                if (!(a <= c)) r0 = c, r1 = a, r2 = b;
            } else {
                if (b <= c) r0 = b, r1 = c, r2 = a;
                else r0 = c, r1 = a, r2 = b;
            }
        }
        k[0] = (uint32_t)r0;
        k[1] = (uint32_t)r1;
        k[2] = (uint32_t)r2;
        return kKeyed;
    }
};

template <typename K>
__global__ void RepLookupKernel(K keys, int64_t n,
                                const int32_t* __restrict__ table,
                                uint32_t slot_mask, int32_t* __restrict__ rep,
                                int32_t* __restrict__ first) {
    O3DMI_GRID_STRIDE(i, n) {
        typename K::Word k[3];
        const int state = keys(i, k);
        const int32_t r = state == kKeyed
                                  ? RepFind(keys, i, k, table, slot_mask)
                                  : (int32_t)i;
        rep[i] = r;
        first[i] = state != kNoKey && r == (int32_t)i;
    }
}

template <typename K>
int RepAsync(const K& keys, int64_t n, int32_t* table_dev, int64_t slots,
             int32_t* rep_dev, int32_t* first_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    O3DMI_REQUIRE(n < kRepMaxRows, "too many rows for the table (< 2^30)");
    O3DMI_REQUIRE(slots >= 2 * n && (slots & (slots - 1)) == 0,
                  "representative table: bad capacity");
    O3DMI_HIP_CHECK(hipMemsetAsync(table_dev, 0xFF,
                                   sizeof(int32_t) * (size_t)slots, s));
    const uint32_t slot_mask = (uint32_t)(slots - 1);
    O3DMI_LAUNCH(RepInsertKernel<K>, n, keys, n, table_dev, slot_mask);
    O3DMI_LAUNCH(RepLookupKernel<K>, n, keys, n, table_dev, slot_mask, rep_dev,
                 first_dev);
    return O3DMI_OK;
}

__global__ void RankOfRepKernel(const int32_t* __restrict__ rep,
                                const int64_t* __restrict__ rank, int64_t n,
                                int64_t* __restrict__ out) {
    O3DMI_GRID_STRIDE(i, n) out[i] = rank[rep[i]];
}

// ---- triangle compaction ------------------------------------------------------------
__global__ void NonDegenerateFlagsKernel(const int32_t* __restrict__ tri,
                                         int64_t m,
                                         int32_t* __restrict__ flags) {
    O3DMI_GRID_STRIDE(t, m) {
        const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        flags[t] = a != b && b != c && c != a;
    }
}

template <typename I>
__global__ void CompactTrianglesKernel(const int32_t* __restrict__ tri,
                                       int64_t m,
                                       const int32_t* __restrict__ flags,
                                       const int64_t* __restrict__ pos,
                                       I* __restrict__ out) {
    O3DMI_GRID_STRIDE(t, m) {
        if (!flags[t]) continue;
        const int64_t p = pos[t];
        out[3 * p] = (I)tri[3 * t];
        out[3 * p + 1] = (I)tri[3 * t + 1];
        out[3 * p + 2] = (I)tri[3 * t + 2];
    }
}

// ---- CSR adjacency --------------------------------------------------------------------
__global__ void EdgeRunFlagsKernel(EdgeTable tb, int64_t n3,
                                   int32_t* __restrict__ flags,
                                   unsigned long long* n_self) {
    unsigned long long mine = 0;
    O3DMI_GRID_STRIDE(j, n3) {
        const bool first = FirstOfRun(tb, j);
        flags[j] = first;
        mine += first && tb.lo[j] == tb.hi[j];
    }
    if (mine) atomicAdd(n_self, mine);
}

__global__ void UniqueEdgesKernel(EdgeTable tb, int64_t n3,
                                  const int32_t* __restrict__ flags,
                                  const int64_t* __restrict__ pos,
                                  uint32_t* __restrict__ lo_out,
                                  uint32_t* __restrict__ hi_out,
                                  int32_t* __restrict__ upper,
                                  int32_t* __restrict__ lower) {
    O3DMI_GRID_STRIDE(j, n3) {
        if (!flags[j]) continue;
        const uint32_t lo = tb.lo[j], hi = tb.hi[j];
        lo_out[pos[j]] = lo;
        hi_out[pos[j]] = hi;
        atomicAdd(&upper[lo], 1);
        if (lo != hi) atomicAdd(&lower[hi], 1);
    }
}

__global__ void AdjacencyRowsKernel(const int64_t* __restrict__ lower_start,
                                    const int64_t* __restrict__ upper_start,
                                    int64_t v, int64_t n_entries,
                                    int64_t* __restrict__ row_splits) {
    O3DMI_GRID_STRIDE(u, v + 1)
        row_splits[u] = u < v ? lower_start[u] + upper_start[u] : n_entries;
}

template <typename I>
__global__ void AdjacencyUpperKernel(const uint32_t* __restrict__ lo,
                                     const uint32_t* __restrict__ hi,
                                     int64_t n_edges,
                                     const int64_t* __restrict__ row_splits,
                                     const int32_t* __restrict__ lower,
                                     const int64_t* __restrict__ upper_start,
                                     I* __restrict__ out) {
    O3DMI_GRID_STRIDE(j, n_edges) {
        const uint32_t u = lo[j];
        out[row_splits[u] + lower[u] + (j - upper_start[u])] = (I)hi[j];
    }
}

__global__ void ByHiPairsKernel(const uint32_t* __restrict__ lo,
                                const uint32_t* __restrict__ hi,
                                int64_t n_edges, uint32_t v,
                                uint32_t* __restrict__ keys,
                                uint32_t* __restrict__ vals) {
    O3DMI_GRID_STRIDE(j, n_edges) {
        keys[j] = lo[j] == hi[j] ? v : hi[j];
        vals[j] = lo[j];
    }
}

template <typename I>
__global__ void AdjacencyLowerKernel(const uint32_t* __restrict__ keys,
                                     const uint32_t* __restrict__ vals,
                                     int64_t n_edges, uint32_t v,
                                     const int64_t* __restrict__ row_splits,
                                     const int64_t* __restrict__ lower_start,
                                     I* __restrict__ out) {
    O3DMI_GRID_STRIDE(j, n_edges) {
        const uint32_t u = keys[j];
        if (u >= v) continue;  // the self edges, behind every vertex
        out[row_splits[u] + (j - lower_start[u])] = (I)vals[j];
    }
}

// ---- vertex clustering ------------------------------------------------------------------
struct Bound3 {
    double x[3];
};

template <typename T>
__global__ void VoxelIndicesKernel(const T* __restrict__ p, int64_t v,
                                   Bound3 min_bound, double voxel_size,
                                   int32_t* __restrict__ vox) {
    O3DMI_GRID_STRIDE(i, 3 * v) {
        const double ref = ((double)p[i] - min_bound.x[i % 3]) / voxel_size;
        vox[i] = (int)floor(ref);
    }
}

__global__ void ClusterPairsKernel(const int64_t* __restrict__ new_index,
                                   int64_t v, uint32_t* __restrict__ keys,
                                   uint32_t* __restrict__ vals,
                                   int32_t* __restrict__ counts) {
    O3DMI_GRID_STRIDE(i, v) {
        const uint32_t c = (uint32_t)new_index[i];
        keys[i] = c;
        vals[i] = (uint32_t)i;
        atomicAdd(&counts[c], 1);
    }
}

// geometry/TriangleMesh.cpp:1248-1262.
template <typename T>
__global__ void TrianglePlanesKernel(const T* __restrict__ pos,
                                     const int32_t* __restrict__ tri,
                                     int64_t m, double* __restrict__ out) {
    O3DMI_GRID_STRIDE(t, m) {
        const int64_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
        double p0[3], e0[3], e1[3];
        for (int k = 0; k < 3; ++k) {
            p0[k] = (double)pos[3 * i0 + k];
            e0[k] = (double)pos[3 * i1 + k] - p0[k];
            e1[k] = (double)pos[3 * i2 + k] - p0[k];
        }
        double abc[3] = {e0[1] * e1[2] - e0[2] * e1[1],
                         e0[2] * e1[0] - e0[0] * e1[2],
                         e0[0] * e1[1] - e0[1] * e1[0]};
        const double norm =
                sqrt((abc[0] * abc[0] + abc[1] * abc[1]) + abc[2] * abc[2]);
        double plane[4] = {0, 0, 0, 0};
        if (!(norm == 0)) {
            for (int k = 0; k < 3; ++k) plane[k] = abc[k] / norm;
            plane[3] = -((plane[0] * p0[0] + plane[1] * p0[1]) +
                         plane[2] * p0[2]);
        }
        for (int k = 0; k < 4; ++k) out[4 * t + k] = plane[k];
    }
}

// Quadric(plane, area) as its 12 addends: A_ij = (w n_i) n_j row-major, then
// b_i = (w d) n_i (TriangleMeshSimplification.cpp:30-35; c is never read).
__device__ __forceinline__ void QuadricTerms(const double plane[4], double w,
                                             double e[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double wn = w * plane[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) e[3 * i + j] = wn * plane[j];
    }
    const double wd = w * plane[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) e[9 + i] = wd * plane[i];
}

// The minimiser of the summed quadric q (A row-major, then b) when it is
// invertible.
__device__ __forceinline__ bool QuadricMinimum(const double q[12],
                                               double x[3]) {
    const double a00 = q[0], a01 = q[1], a02 = q[2], a10 = q[3], a11 = q[4],
                 a12 = q[5], a20 = q[6], a21 = q[7], a22 = q[8];
    const double m00 = a11 * a22 - a12 * a21, m01 = a10 * a22 - a12 * a20,
                 m02 = a10 * a21 - a11 * a20;
    const double det = a00 * m00 - a01 * m01 + a02 * m02;
    if (!(fabs(det) > 1e-4)) return false;
    const double c[3][3] = {
            {m00, -m01, m02},
            {-(a01 * a22 - a02 * a21), a00 * a22 - a02 * a20,
             -(a00 * a21 - a01 * a20)},
            {a01 * a12 - a02 * a11, -(a00 * a12 - a02 * a10),
             a00 * a11 - a01 * a10}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
        x[i] = -((c[i][0] * q[9] + c[i][1] * q[10]) + c[i][2] * q[11]) / det;
    return true;
}

template <typename T>
__device__ __forceinline__ void StoreRow(void* out, int64_t row,
                                         const double x[3]) {
    T* o = (T*)out + 3 * row;
    o[0] = (T)x[0];
    o[1] = (T)x[1];
    o[2] = (T)x[2];
}

// The outputs of cluster c from its sums (every lane of a wave may call it
// with the same values; `store` picks the one that writes).
template <typename T>
__device__ __forceinline__ void StoreCluster(const ClusterIO& io, int64_t c,
                                             int cnt, const double sp[3],
                                             const double sn[3],
                                             const double sc[3],
                                             const double q[12], bool store) {
    const double n = (double)cnt;
    double x[3];
    if (!(io.quadric && QuadricMinimum(q, x)))
        for (int k = 0; k < 3; ++k) x[k] = sp[k] / n;
    if (!store) return;
    StoreRow<T>(io.positions_out, c, x);
    if (io.normals) {
        const double a[3] = {sn[0] / n, sn[1] / n, sn[2] / n};
        StoreRow<T>(io.normals_out, c, a);
    }
    if (io.colors) {
        const double a[3] = {sc[0] / n, sc[1] / n, sc[2] / n};
        StoreRow<T>(io.colors_out, c, a);
    }
}

template <typename T>
__global__ void ContractThreadKernel(ClusterIO io, int64_t n_clusters,
                                     int32_t* __restrict__ long_list) {
    const T* pos = (const T*)io.positions;
    const T* nrm = (const T*)io.normals;
    const T* col = (const T*)io.colors;
    O3DMI_GRID_STRIDE(c, n_clusters) {
        const int cnt = io.counts[c];
        if (cnt > kLongCornerList) {
            long_list[atomicAdd(&long_list[n_clusters], 1)] = (int32_t)c;
            continue;
        }
        const uint32_t* mem = io.members + io.start[c];
        double sp[3] = {0, 0, 0}, sn[3] = {0, 0, 0}, sc[3] = {0, 0, 0};
        double q[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4  // the loads do not depend on the adds
        for (int j = 0; j < cnt; ++j) {
            const int64_t i = mem[j];
            for (int k = 0; k < 3; ++k) {
                sp[k] += (double)pos[3 * i + k];
                if (nrm) sn[k] += (double)nrm[3 * i + k];
                if (col) sc[k] += (double)col[3 * i + k];
            }
        }
        if (io.quadric) {
            for (int j = 0; j < cnt; ++j) {
                const int64_t i = mem[j];
                const int n_corners = io.corners.count[i];
                const uint32_t* corner = io.corners.corner + io.corners.start[i];
                uint32_t before = 0xFFFFFFFFu;
                for (int k = 0; k < n_corners; ++k) {
                    const uint32_t t = corner[k] / 3u;
                    // a triangle that names the vertex twice counts once
                    if (t == before) continue;
                    before = t;
                    const double* pl = io.plane + 4 * (int64_t)t;
                    const double plane[4] = {pl[0], pl[1], pl[2], pl[3]};
                    double e[12];
                    QuadricTerms(plane, io.area[t], e);
#pragma unroll
                    for (int x = 0; x < 12; ++x) q[x] += e[x];
                }
            }
        }
        StoreCluster<T>(io, c, cnt, sp, sn, sc, q, true);
    }
}

// A wave per listed cluster: 64 members' rows are fetched at once and added
// in member order; for the quadric the members are then taken one by one and
// 64 of a member's corners fetched at once, their terms added in corner
// order. Every lane does the same adds; lane 0 stores.
template <typename T>
__global__ void ContractWaveKernel(ClusterIO io, int64_t n_clusters,
                                   const int32_t* __restrict__ long_list) {
    const T* pos = (const T*)io.positions;
    const T* nrm = (const T*)io.normals;
    const T* col = (const T*)io.colors;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int n_long = long_list[n_clusters];
    for (int64_t w = wave; w < n_long; w += n_waves) {
        const int64_t c = long_list[w];
        const int cnt = io.counts[c];
        const uint32_t* mem = io.members + io.start[c];
        double sp[3] = {0, 0, 0}, sn[3] = {0, 0, 0}, sc[3] = {0, 0, 0};
        double q[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            double p[3] = {0, 0, 0}, a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
            int n_corners = 0;
            long long corner_start = 0;
            if (j0 + lane < cnt) {
                const int64_t i = mem[j0 + lane];
                for (int k = 0; k < 3; ++k) {
                    p[k] = (double)pos[3 * i + k];
                    if (nrm) a[k] = (double)nrm[3 * i + k];
                    if (col) b[k] = (double)col[3 * i + k];
                }
                if (io.quadric) {
                    n_corners = io.corners.count[i];
                    corner_start = io.corners.start[i];
                }
            }
            const int len = cnt - j0 < 64 ? cnt - j0 : 64;
            for (int l = 0; l < len; ++l) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    sp[k] += __shfl(p[k], l);
                    if (nrm) sn[k] += __shfl(a[k], l);
                    if (col) sc[k] += __shfl(b[k], l);
                }
            }
            if (!io.quadric) continue;
            for (int l = 0; l < len; ++l) {
                const int nc = __shfl(n_corners, l);
                const uint32_t* corner =
                        io.corners.corner + __shfl(corner_start, l);
                for (int k0 = 0; k0 < nc; k0 += 64) {
                    double e[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                    int skip = 1;
                    const int k = k0 + lane;
                    if (k < nc) {
                        const uint32_t t = corner[k] / 3u;
                        skip = k > 0 && corner[k - 1] / 3u == t;
                        const double* pl = io.plane + 4 * (int64_t)t;
                        const double plane[4] = {pl[0], pl[1], pl[2], pl[3]};
                        QuadricTerms(plane, io.area[t], e);
                    }
                    const int klen = nc - k0 < 64 ? nc - k0 : 64;
                    for (int kk = 0; kk < klen; ++kk) {
                        if (__shfl(skip, kk)) continue;  // the same in all lanes
#pragma unroll
                        for (int x = 0; x < 12; ++x) q[x] += __shfl(e[x], kk);
                    }
                }
            }
        }
        StoreCluster<T>(io, c, cnt, sp, sn, sc, q, lane == 0);
    }
}

// TriangleMeshSimplification.cpp:206-227.
__global__ void MapClusterTrianglesKernel(const int32_t* __restrict__ tri,
                                          int64_t m,
                                          const int64_t* __restrict__ new_index,
                                          int32_t* __restrict__ mapped) {
    O3DMI_GRID_STRIDE(t, m) {
        int32_t v0 = (int32_t)new_index[tri[3 * t]];
        int32_t v1 = (int32_t)new_index[tri[3 * t + 1]];
        int32_t v2 = (int32_t)new_index[tri[3 * t + 2]];
        if (v0 == v1 || v0 == v2 || v1 == v2) {
            v0 = v1 = v2 = -1;
        } else if (v1 < v0 && v1 < v2) {
            const int32_t tmp = v0;
            v0 = v1;
            v1 = v2;
            v2 = tmp;
        } else if (v2 < v0 && v2 < v1) {
            const int32_t tmp = v1;
            v1 = v0;
            v0 = v2;
            v2 = tmp;
        }
        mapped[3 * t] = v0;
        mapped[3 * t + 1] = v1;
        mapped[3 * t + 2] = v2;
    }
}

}  // namespace

int64_t RepTableSlots(int64_t n) {
    int64_t slots = 64;
    while (slots < 2 * n) slots <<= 1;
    return slots;
}

int VertexRepAsync(const void* positions_dev, int64_t v, int dtype,
                   int32_t* table_dev, int64_t slots, int32_t* rep_dev,
                   int32_t* first_dev, hipStream_t s) {
    if (dtype == O3DMI_F64)
        return RepAsync(
                VertexKeys<double, uint64_t>{(const double*)positions_dev}, v,
                table_dev, slots, rep_dev, first_dev, s);
    return RepAsync(VertexKeys<float, uint32_t>{(const float*)positions_dev}, v,
                    table_dev, slots, rep_dev, first_dev, s);
}

int TripleRepAsync(const int32_t* triples_dev, int64_t n, bool rotate,
                   int32_t* table_dev, int64_t slots, int32_t* rep_dev,
                   int32_t* first_dev, hipStream_t s) {
    return RepAsync(TripleKeys{triples_dev, rotate}, n, table_dev, slots,
                    rep_dev, first_dev, s);
}

int RankOfRepAsync(const int32_t* rep_dev, const int64_t* rank_dev, int64_t n,
                   int64_t* out_dev, hipStream_t s) {
    O3DMI_LAUNCH(RankOfRepKernel, n, rep_dev, rank_dev, n, out_dev);
    return O3DMI_OK;
}

int NonDegenerateFlagsAsync(const int32_t* tri, int64_t m, int32_t* flags_dev,
                            hipStream_t s) {
    O3DMI_LAUNCH(NonDegenerateFlagsKernel, m, tri, m, flags_dev);
    return O3DMI_OK;
}

int CompactTrianglesAsync(const int32_t* tri, int64_t m,
                          const int32_t* flags_dev, const int64_t* pos_dev,
                          int index_dtype, void* out_dev, hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(CompactTrianglesKernel<int64_t>, m, tri, m, flags_dev,
                     pos_dev, (int64_t*)out_dev);
    else
        O3DMI_LAUNCH(CompactTrianglesKernel<int32_t>, m, tri, m, flags_dev,
                     pos_dev, (int32_t*)out_dev);
    return O3DMI_OK;
}

int EdgeRunFlagsAsync(const EdgeTable& table, int64_t n_slots,
                      int32_t* flags_dev, unsigned long long* n_self_dev,
                      hipStream_t s) {
    O3DMI_LAUNCH(EdgeRunFlagsKernel, n_slots, table, n_slots, flags_dev,
                 n_self_dev);
    return O3DMI_OK;
}

int UniqueEdgesAsync(const EdgeTable& table, int64_t n_slots,
                     const int32_t* flags_dev, const int64_t* pos_dev,
                     uint32_t* lo_out_dev, uint32_t* hi_out_dev,
                     int32_t* upper_dev, int32_t* lower_dev, hipStream_t s) {
    O3DMI_LAUNCH(UniqueEdgesKernel, n_slots, table, n_slots, flags_dev, pos_dev,
                 lo_out_dev, hi_out_dev, upper_dev, lower_dev);
    return O3DMI_OK;
}

int AdjacencyRowsAsync(const int64_t* lower_start_dev,
                       const int64_t* upper_start_dev, int64_t v,
                       int64_t n_entries, int64_t* row_splits_dev,
                       hipStream_t s) {
    O3DMI_LAUNCH(AdjacencyRowsKernel, v + 1, lower_start_dev, upper_start_dev,
                 v, n_entries, row_splits_dev);
    return O3DMI_OK;
}

int AdjacencyUpperAsync(const uint32_t* lo_dev, const uint32_t* hi_dev,
                        int64_t n_edges, const int64_t* row_splits_dev,
                        const int32_t* lower_dev,
                        const int64_t* upper_start_dev, int index_dtype,
                        void* neighbours_dev, hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(AdjacencyUpperKernel<int64_t>, n_edges, lo_dev, hi_dev,
                     n_edges, row_splits_dev, lower_dev, upper_start_dev,
                     (int64_t*)neighbours_dev);
    else
        O3DMI_LAUNCH(AdjacencyUpperKernel<int32_t>, n_edges, lo_dev, hi_dev,
                     n_edges, row_splits_dev, lower_dev, upper_start_dev,
                     (int32_t*)neighbours_dev);
    return O3DMI_OK;
}

int ByHiPairsAsync(const uint32_t* lo_dev, const uint32_t* hi_dev,
                   int64_t n_edges, int64_t v, uint32_t* keys_dev,
                   uint32_t* vals_dev, hipStream_t s) {
    O3DMI_LAUNCH(ByHiPairsKernel, n_edges, lo_dev, hi_dev, n_edges,
                 (uint32_t)v, keys_dev, vals_dev);
    return O3DMI_OK;
}

int AdjacencyLowerAsync(const uint32_t* keys_dev, const uint32_t* vals_dev,
                        int64_t n_edges, int64_t v,
                        const int64_t* row_splits_dev,
                        const int64_t* lower_start_dev, int index_dtype,
                        void* neighbours_dev, hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(AdjacencyLowerKernel<int64_t>, n_edges, keys_dev,
                     vals_dev, n_edges, (uint32_t)v, row_splits_dev,
                     lower_start_dev, (int64_t*)neighbours_dev);
    else
        O3DMI_LAUNCH(AdjacencyLowerKernel<int32_t>, n_edges, keys_dev,
                     vals_dev, n_edges, (uint32_t)v, row_splits_dev,
                     lower_start_dev, (int32_t*)neighbours_dev);
    return O3DMI_OK;
}

int VoxelIndicesAsync(const void* positions_dev, int64_t v, int dtype,
                      const double min_bound[3], double voxel_size,
                      int32_t* vox_dev, hipStream_t s) {
    const Bound3 b = {{min_bound[0], min_bound[1], min_bound[2]}};
    if (dtype == O3DMI_F64)
        O3DMI_LAUNCH(VoxelIndicesKernel<double>, 3 * v,
                     (const double*)positions_dev, v, b, voxel_size, vox_dev);
    else
        O3DMI_LAUNCH(VoxelIndicesKernel<float>, 3 * v,
                     (const float*)positions_dev, v, b, voxel_size, vox_dev);
    return O3DMI_OK;
}

int ClusterPairsAsync(const int64_t* new_index_dev, int64_t v,
                      uint32_t* keys_dev, uint32_t* vals_dev,
                      int32_t* counts_dev, hipStream_t s) {
    O3DMI_LAUNCH(ClusterPairsKernel, v, new_index_dev, v, keys_dev, vals_dev,
                 counts_dev);
    return O3DMI_OK;
}

int TrianglePlanesAsync(const void* positions_dev, int dtype,
                        const int32_t* tri, int64_t m, double* plane_out_dev,
                        hipStream_t s) {
    if (dtype == O3DMI_F64)
        O3DMI_LAUNCH(TrianglePlanesKernel<double>, m,
                     (const double*)positions_dev, tri, m, plane_out_dev);
    else
        O3DMI_LAUNCH(TrianglePlanesKernel<float>, m,
                     (const float*)positions_dev, tri, m, plane_out_dev);
    return O3DMI_OK;
}

int ContractClustersAsync(const ClusterIO& io, int64_t n_clusters, int dtype,
                          int32_t* long_list_dev, hipStream_t s) {
    const dim3 waves = WaveGrid(n_clusters);
    if (dtype == O3DMI_F64) {
        O3DMI_LAUNCH(ContractThreadKernel<double>, n_clusters, io, n_clusters,
                     long_list_dev);
        hipLaunchKernelGGL(ContractWaveKernel<double>, waves, dim3(kBlock), 0,
                           s, io, n_clusters, long_list_dev);
    } else {
        O3DMI_LAUNCH(ContractThreadKernel<float>, n_clusters, io, n_clusters,
                     long_list_dev);
        hipLaunchKernelGGL(ContractWaveKernel<float>, waves, dim3(kBlock), 0,
                           s, io, n_clusters, long_list_dev);
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int MapClusterTrianglesAsync(const int32_t* tri, int64_t m,
                             const int64_t* new_index_dev, int32_t* mapped_dev,
                             hipStream_t s) {
    O3DMI_LAUNCH(MapClusterTrianglesKernel, m, tri, m, new_index_dev,
                 mapped_dev);
    return O3DMI_OK;
}

}  // namespace o3dmi
