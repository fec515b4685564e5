// FPFH features and feature-space nearest neighbours
// (t/pipelines/kernel/FeatureImpl.h:25-296, t/pipelines/registration/
// Feature.cpp:279-333).
//
// FPFH: two passes over neighbour lists, one lane per row. A row's sums run in
// neighbour-list order inside one lane, so the same point gives the same bits
// whether it is computed in the whole cloud or through an `indices` subset.
//   SpfhKernel: the pair features of a point's list positions 1..count-1, each
//     adding hist_incr to three of the row's 33 bins. The row lives in LDS
//     (bin-major, lane fastest) while it is built: bins are picked at run
//     time, and a register array indexed that way would go to scratch.
//   FpfhKernel: the d2-weighted sum of the neighbours' SPFH rows (unrolled
//     over the 33 bins: registers), normalised per 11-bin group, plus the
//     point's own SPFH.
//
// Correspondences: exact 1-NN in feature space. The distance of rows a, b is
// sum_k (a_k - b_k)^2 in float64, k ascending, no FMA; the smallest distance
// wins, ties go to the lowest index, a NaN distance counts as +inf (so every
// row gets an index in range). Nn1Kernel evaluates exactly that on the
// float64 VALU, 64 x 64 pairs per workgroup and 4 x 4 per lane, with both
// tiles staged in LDS in chunks of kNnKc dimensions (zero padding adds exact
// zeros). Target slices run in separate workgroups and are merged in slice
// order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "common.h"
#include "feature.h"
#include "scan.h"

using namespace o3dmi;

namespace {

constexpr int kFeat = 33;
constexpr int kSpfhBlock = 64;

template <typename T>
__device__ __forceinline__ T Dot3(const T* a, const T* b) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

template <typename T>
__device__ __forceinline__ void Cross3(const T* a, const T* b, T* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// ComputePairFeature (FeatureImpl.h:25-86), same operations in scalar_t.
template <typename T>
__device__ __forceinline__ void PairFeature(const T* p1, const T* n1,
                                            const T* p2, const T* n2, T* f) {
    T dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    f[3] = sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]);
    if (f[3] == 0) {
        f[0] = f[1] = f[2] = f[3] = 0;
        return;
    }
    const T angle1 = Dot3(n1, dp) / f[3];
    const T angle2 = Dot3(n2, dp) / f[3];
    T a[3], b[3];
    if (acos(fabs(angle1)) > acos(fabs(angle2))) {
        a[0] = n2[0]; a[1] = n2[1]; a[2] = n2[2];
        b[0] = n1[0]; b[1] = n1[1]; b[2] = n1[2];
        dp[0] *= -1;
        dp[1] *= -1;
        dp[2] *= -1;
        f[2] = -angle2;
    } else {
        a[0] = n1[0]; a[1] = n1[1]; a[2] = n1[2];
        b[0] = n2[0]; b[1] = n2[1]; b[2] = n2[2];
        f[2] = angle1;
    }
    T v[3];
    Cross3(dp, a, v);
    const T v_norm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (v_norm == 0.0) {
        f[0] = f[1] = f[2] = f[3] = 0;
        return;
    }
    v[0] /= v_norm;
    v[1] /= v_norm;
    v[2] /= v_norm;
    T w[3];
    Cross3(a, v, w);
    f[1] = Dot3(v, b);
    f[0] = atan2(Dot3(w, b), Dot3(a, b));
}

// UpdateSPFHFeature's bins (FeatureImpl.h:88-106): float64, as M_PI forces.
__device__ __forceinline__ int Bin(double x) {
    const int h = (int)floor(x);
    return h >= 11 ? 10 : (h > 0 ? h : 0);
}

// A row's neighbour list: padded {rows, nn} with counts, or CSR splits.
struct Lists {
    const int32_t* idx;
    const int32_t* counts;     // padded form
    const int64_t* splits;     // CSR form (counts == NULL)
    int nn;
    __device__ __forceinline__ void Row(int64_t r, int64_t& base,
                                        int& count) const {
        if (counts) {
            base = r * nn;
            count = counts[r];
        } else {
            base = splits[r];
            count = (int)(splits[r + 1] - base);
        }
    }
};

template <typename T>
__global__ void __launch_bounds__(kSpfhBlock)
SpfhKernel(const T* __restrict__ pts, const T* __restrict__ nrm, Lists lists,
           const int64_t* __restrict__ row_point, int64_t n_rows,
           T* __restrict__ spfh) {
    __shared__ T hist[kFeat][kSpfhBlock];
    const int lane = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * kSpfhBlock + lane;
    if (r >= n_rows) return;  // lanes own their LDS column: no barrier needed
#pragma unroll
    for (int j = 0; j < kFeat; ++j) hist[j][lane] = T(0);
    const int64_t p = row_point ? row_point[r] : r;
    const T p1[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
    const T n1[3] = {nrm[3 * p], nrm[3 * p + 1], nrm[3 * p + 2]};
    int64_t base;
    int count;
    lists.Row(r, base, count);
    if (count > 1) {
        const T incr = (T)(100.0 / (double)(T)(count - 1));
        for (int i = 1; i < count; ++i) {
            const int64_t q = lists.idx[base + i];
            const T p2[3] = {pts[3 * q], pts[3 * q + 1], pts[3 * q + 2]};
            const T n2[3] = {nrm[3 * q], nrm[3 * q + 1], nrm[3 * q + 2]};
            T f[4];
            PairFeature(p1, n1, p2, n2, f);
            const int h1 = Bin(11 * ((double)f[0] + M_PI) / (2.0 * M_PI));
            const int h2 = Bin(11 * ((double)f[1] + 1.0) * 0.5);
            const int h3 = Bin(11 * ((double)f[2] + 1.0) * 0.5);
            hist[h1][lane] += incr;
            hist[h2 + 11][lane] += incr;
            hist[h3 + 22][lane] += incr;
        }
    }
    T* out = spfh + r * kFeat;
#pragma unroll
    for (int j = 0; j < kFeat; ++j) out[j] = hist[j][lane];
}

// Pass 2 (FeatureImpl.h:248-288). Output row o is point fpfh_point[o] (NULL:
// o) whose lists / SPFH row is point_row[point] (NULL: the point itself).
constexpr int kFpfhBlock = 128;

template <typename T>
__global__ void __launch_bounds__(kFpfhBlock)
FpfhKernel(const T* __restrict__ dist2, Lists lists,
                           const T* __restrict__ spfh,
                           const int32_t* __restrict__ fpfh_point,
                           const int32_t* __restrict__ point_row,
                           int64_t n_out, T* __restrict__ fpfh) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_out) return;
    const int64_t p = fpfh_point ? fpfh_point[o] : o;
    const int64_t s = point_row ? point_row[p] : p;
    int64_t base;
    int count;
    lists.Row(s, base, count);
    T acc[kFeat];
#pragma unroll
    for (int j = 0; j < kFeat; ++j) acc[j] = T(0);
    T* out = fpfh + o * kFeat;
    if (count > 1) {
        T sum[3] = {T(0), T(0), T(0)};
        for (int i = 1; i < count; ++i) {
            const T d = dist2[base + i];
            if (d == 0.0) continue;
            const int64_t q = lists.idx[base + i];
            const T* row = spfh + (point_row ? point_row[q] : q) * kFeat;
#pragma unroll
            for (int j = 0; j < kFeat; ++j) {
                const T val = row[j] / d;
                sum[j / 11] += val;
                acc[j] += val;
            }
        }
#pragma unroll
        for (int g = 0; g < 3; ++g)
            sum[g] = sum[g] != 0.0 ? (T)(100.0 / (double)sum[g]) : T(0);
        const T* own = spfh + s * kFeat;
#pragma unroll
        for (int j = 0; j < kFeat; ++j) {
            acc[j] *= sum[j / 11];
            acc[j] += own[j];
        }
    }
#pragma unroll
    for (int j = 0; j < kFeat; ++j) out[j] = acc[j];
}

__global__ void MaskToIntKernel(const uint8_t* __restrict__ mask, int64_t n,
                                int32_t* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        out[i] = mask[i] ? 1 : 0;
}

// NonZero(mask) through an exclusive scan: list[pos[i]] = i.
__global__ void CompactKernel(const uint8_t* __restrict__ mask,
                              const int64_t* __restrict__ pos, int64_t n,
                              int32_t* __restrict__ list) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        if (mask[i]) list[pos[i]] = (int32_t)i;
}

__global__ void FillKernel(int32_t* __restrict__ a, int64_t n, int32_t v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        a[i] = v;
}

__global__ void InverseMapKernel(const int64_t* __restrict__ row_point,
                                 int64_t n_rows, int64_t n_points,
                                 int32_t* __restrict__ point_row,
                                 int* __restrict__ bad) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = row_point[r];
        if (p < 0 || p >= n_points) {
            *bad = 1;
            continue;
        }
        point_row[p] = (int32_t)r;
    }
}

// Every neighbour of a requested row must have an SPFH row.
__global__ void CheckRowsKernel(const int32_t* __restrict__ fpfh_point,
                                int64_t n_out, const int32_t* __restrict__ point_row,
                                int64_t n_points, Lists lists,
                                int* __restrict__ bad) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_out) return;
    const int32_t s = point_row[fpfh_point[o]];
    if (s < 0) {
        *bad = 1;
        return;
    }
    int64_t base;
    int count;
    lists.Row(s, base, count);
    for (int i = 1; i < count; ++i) {
        const int32_t q = lists.idx[base + i];
        if (q < 0 || q >= n_points || point_row[q] < 0) *bad = 1;
    }
}

// ---- exact 1-NN in feature space --------------------------------------------
constexpr int kNnTile = 64;   // rows and columns of a workgroup tile
constexpr int kNnKc = 12;     // dimensions per LDS chunk
constexpr int kNnBlock = 256; // 16 x 16 lanes, 4 x 4 pairs each

template <typename T>
__device__ __forceinline__ void LoadTile(const T* __restrict__ x, int64_t n,
                                         int dim, int64_t r0, int k0,
                                         double (*tile)[kNnTile + 2]) {
    for (int e = threadIdx.x; e < kNnTile * kNnKc; e += kNnBlock) {
        const int r = e / kNnKc, k = e % kNnKc;
        const int64_t row = r0 + r;
        const int kk = k0 + k;
        tile[k][r] = (row < n && kk < dim) ? (double)x[row * dim + kk] : 0.0;
    }
}

__device__ __forceinline__ bool Before(double ad, int ai, double bd, int bi) {
    return ad < bd || (ad == bd && ai < bi);
}

// A NaN distance (a NaN or inf feature) counts as +inf: every row still gets
// an index in range, the lowest among its equal (possibly all +inf) distances.
__device__ __forceinline__ double OrderKey(double d) {
    return d != d ? (double)INFINITY : d;
}

// For rows [64 bx, +64) of a: the nearest row of b among columns
// [slice * cols_per_slice, +cols_per_slice); written to part_{d,i}[slice][row].
template <typename T>
__global__ void __launch_bounds__(kNnBlock)
Nn1Kernel(const T* __restrict__ a, int64_t na, const T* __restrict__ b,
          int64_t nb, int dim, int64_t cols_per_slice,
          double* __restrict__ part_d, int32_t* __restrict__ part_i) {
    __shared__ double ta[kNnKc][kNnTile + 2];
    __shared__ double tb[kNnKc][kNnTile + 2];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * kNnTile;
    const int64_t c_begin = (int64_t)blockIdx.y * cols_per_slice;
    int64_t c_end = c_begin + cols_per_slice;
    if (c_end > nb) c_end = nb;
    double best_d[4];
    int best_i[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        best_d[r] = INFINITY;
        best_i[r] = 0x7fffffff;
    }
    for (int64_t c0 = c_begin; c0 < c_end; c0 += kNnTile) {
        double acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
        for (int k0 = 0; k0 < dim; k0 += kNnKc) {
            __syncthreads();
            LoadTile(a, na, dim, r0, k0, ta);
            LoadTile(b, c_end, dim, c0, k0, tb);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kNnKc; ++k) {
                double av[4], bv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) av[r] = ta[k][ty * 4 + r];
#pragma unroll
                for (int c = 0; c < 4; ++c) bv[c] = tb[k][tx * 4 + c];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const double d = av[r] - bv[c];
                        acc[r][c] = acc[r][c] + d * d;
                    }
            }
        }
        // columns of this lane in ascending order
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t j = c0 + tx * 4 + c;
            if (j < c_end) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double d = OrderKey(acc[r][c]);
                    // lexicographic: a first +inf still replaces the empty
                    // (+inf, 0x7fffffff) start
                    if (Before(d, (int)j, best_d[r], best_i[r])) {
                        best_d[r] = d;
                        best_i[r] = (int)j;
                    }
                }
            }
        }
    }
    // the 16 lanes of a row group (same ty) are lanes 16*(ty%4) .. +15
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double d = best_d[r];
        int i = best_i[r];
#pragma unroll
        for (int m = 8; m > 0; m >>= 1) {
            const double od = __shfl_xor(d, m, 16);
            const int oi = __shfl_xor(i, m, 16);
            if (Before(od, oi, d, i)) {
                d = od;
                i = oi;
            }
        }
        const int64_t row = r0 + ty * 4 + r;
        if (tx == 0 && row < na) {
            part_d[(int64_t)blockIdx.y * na + row] = d;
            part_i[(int64_t)blockIdx.y * na + row] = i;
        }
    }
}

// Slice minima in slice order; ties keep the lower index.
__global__ void Nn1MergeKernel(const double* __restrict__ part_d,
                               const int32_t* __restrict__ part_i, int64_t na,
                               int slices, int32_t* __restrict__ out) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < na;
         r += (int64_t)gridDim.x * blockDim.x) {
        double d = part_d[r];
        int i = part_i[r];
        for (int s = 1; s < slices; ++s) {
            const double od = part_d[(int64_t)s * na + r];
            const int oi = part_i[(int64_t)s * na + r];
            if (Before(od, oi, d, i)) {
                d = od;
                i = oi;
            }
        }
        out[r] = i;
    }
}

// Feature.cpp:305-332 in one workgroup: keep (i, ij[i]) where ji[ij[i]] == i,
// ascending i; all pairs when the survivors are <= ratio * n (float, as the
// reference's float ratio times the length). info[0] = rows written, info[1] =
// 1 when the fallback was taken.
constexpr int kMutualBlock = 1024;

__global__ void __launch_bounds__(kMutualBlock)
MutualKernel(const int32_t* __restrict__ ij, const int32_t* __restrict__ ji,
             int64_t n, int mutual, float ratio, int64_t* __restrict__ out,
             int64_t* __restrict__ info) {
    __shared__ int64_t wsum[kMutualBlock / 64];
    __shared__ int64_t total_s;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int64_t kept = 0;
    if (mutual) {
        for (int64_t i = threadIdx.x; i < n; i += kMutualBlock)
            kept += ji[ij[i]] == i ? 1 : 0;
        for (int m = 32; m > 0; m >>= 1) kept += __shfl_xor(kept, m);
        if (lane == 0) wsum[wid] = kept;
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t t = 0;
            for (int w = 0; w < kMutualBlock / 64; ++w) t += wsum[w];
            total_s = t;
        }
        __syncthreads();
        kept = total_s;
    }
    const bool filter = mutual && (float)kept > ratio * (float)n;
    int64_t at = 0;
    for (int64_t c0 = 0; c0 < n; c0 += kMutualBlock) {
        const int64_t i = c0 + threadIdx.x;
        const bool keep = i < n && (!filter || ji[ij[i]] == i);
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) wsum[wid] = __popcll(bal);
        __syncthreads();
        int64_t off = at;
        for (int w = 0; w < wid; ++w) off += wsum[w];
        if (keep) {
            out[2 * (off + before)] = i;
            out[2 * (off + before) + 1] = ij[i];
        }
        for (int w = 0; w < kMutualBlock / 64; ++w) at += wsum[w];
    }
    if (threadIdx.x == 0) {
        info[0] = at;
        info[1] = mutual && !filter ? 1 : 0;
    }
}

template <typename T>
int LaunchFpfh(const T* pts, const T* nrm, const T* dist2, Lists lists,
               const int64_t* row_point, int64_t n_rows,
               const int32_t* fpfh_point, const int32_t* point_row,
               int64_t n_out, T* spfh, T* fpfh, hipStream_t s) {
    if (n_rows > 0)
        hipLaunchKernelGGL(SpfhKernel<T>,
                           dim3((unsigned)((n_rows + kSpfhBlock - 1) /
                                           kSpfhBlock)),
                           dim3(kSpfhBlock), 0, s, pts, nrm, lists, row_point,
                           n_rows, spfh);
    if (n_out > 0)
        hipLaunchKernelGGL(FpfhKernel<T>,
                           dim3((unsigned)((n_out + kFpfhBlock - 1) /
                                           kFpfhBlock)),
                           dim3(kFpfhBlock), 0,
                           s, dist2, lists, (const T*)spfh, fpfh_point,
                           point_row, n_out, fpfh);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}


// ---- helpers of the FPFH operator (csrc/host/feature.cpp) -------------------
__global__ void MarkIndicesKernel(const int64_t* __restrict__ idx, int64_t m,
                                  int64_t n, uint8_t* __restrict__ mask,
                                  int* __restrict__ bad) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = idx[i];
        if (p < 0 || p >= n) *bad = 1;
        else mask[p] = 1;
    }
}

__global__ void MarkListsKernel(const int32_t* __restrict__ idx, int64_t m,
                                uint8_t* __restrict__ mask) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
         i += (int64_t)gridDim.x * blockDim.x)
        if (idx[i] >= 0) mask[idx[i]] = 1;
}

__global__ void WidenKernel(const int32_t* __restrict__ a, int64_t n,
                            int64_t* __restrict__ b) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        b[i] = a[i];
}

__global__ void ShortRowsKernel(const int32_t* __restrict__ counts, int64_t n,
                                int k, int32_t* __restrict__ ids,
                                int* __restrict__ n_ids) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        if (counts[i] < k) ids[atomicAdd(n_ids, 1)] = (int32_t)i;
}

__device__ __forceinline__ unsigned long long OrderedKey(double v) {
    unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
inline double FromOrderedKey(unsigned long long u) {
    u = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
    double v;
    std::memcpy(&v, &u, sizeof(v));
    return v;
}

template <typename T>
__global__ void BoundsKernel(const T* __restrict__ pts, int64_t n,
                             unsigned long long* __restrict__ box) {
    double lo[3] = {INFINITY, INFINITY, INFINITY};
    double hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double v = (double)pts[3 * i + a];
            lo[a] = fmin(lo[a], v);
            hi[a] = fmax(hi[a], v);
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int m = 32; m > 0; m >>= 1) {
            lo[a] = fmin(lo[a], __shfl_xor(lo[a], m));
            hi[a] = fmax(hi[a], __shfl_xor(hi[a], m));
        }
        if ((threadIdx.x & 63) == 0 && lo[a] <= hi[a]) {
            atomicMin(&box[a], OrderedKey(lo[a]));
            atomicMax(&box[3 + a], OrderedKey(hi[a]));
        }
    }
}

}  // namespace

extern "C" {

// indices -> mask[n] (set to 1); *bad_dev = 1 for an index outside [0, n).
int o3dmi_internal_fpfh_mark_indices(const int64_t* idx_dev, int64_t m,
                                     int64_t n, uint8_t* mask_dev,
                                     int* bad_dev, o3dmi_stream_t stream) {
    if (m > 0)
        hipLaunchKernelGGL(MarkIndicesKernel, dim3(GridFor(m, kBlock)),
                           dim3(kBlock), 0, (hipStream_t)stream, idx_dev, m, n,
                           mask_dev, bad_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

// every list entry >= 0 -> mask[entry] = 1
int o3dmi_internal_fpfh_mark_lists(const int32_t* idx_dev, int64_t m,
                                   uint8_t* mask_dev, o3dmi_stream_t stream) {
    if (m > 0)
        hipLaunchKernelGGL(MarkListsKernel, dim3(GridFor(m, kBlock)),
                           dim3(kBlock), 0, (hipStream_t)stream, idx_dev, m,
                           mask_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

// NonZero(mask) ascending into list32 (and list64 when given); waits for the
// count.
int o3dmi_internal_mask_nonzero(const uint8_t* mask_dev, int64_t n,
                                int32_t* list32_dev, int64_t* list64_dev,
                                int64_t* count, o3dmi_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    *count = 0;
    if (n == 0) return O3DMI_OK;
    PoolScratch sc(s);
    int32_t* m32 = nullptr;
    int64_t* pos = nullptr;
    void* tmp = nullptr;
    int st;
    if ((st = sc.Alloc(&m32, 4 * (size_t)n)) ||
        (st = sc.Alloc(&pos, 8 * (size_t)(n + 1))) ||
        (st = sc.Alloc(&tmp, ScanScratchBytes(n))))
        return st;
    const dim3 g(GridFor(n, kBlock)), b(kBlock);
    hipLaunchKernelGGL(MaskToIntKernel, g, b, 0, s, mask_dev, n, m32);
    if ((st = PrefixSumAsync(m32, n, false, pos, pos + n, tmp, s))) return st;
    hipLaunchKernelGGL(CompactKernel, g, b, 0, s, mask_dev, pos, n, list32_dev);
    O3DMI_HIP_CHECK(hipMemcpyAsync(count, pos + n, 8, hipMemcpyDeviceToHost,
                                   s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    if (list64_dev && *count > 0)
        hipLaunchKernelGGL(WidenKernel, dim3(GridFor(*count, kBlock)), b, 0, s,
                           list32_dev, *count, list64_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

// rows i < n with counts[i] < k, in any order; waits for their number.
int o3dmi_internal_short_rows(const int32_t* counts_dev, int64_t n, int k,
                              int32_t* ids_dev, int* n_ids_dev, int* n_ids,
                              o3dmi_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    O3DMI_HIP_CHECK(hipMemsetAsync(n_ids_dev, 0, sizeof(int), s));
    if (n > 0)
        hipLaunchKernelGGL(ShortRowsKernel, dim3(GridFor(n, kBlock)),
                           dim3(kBlock), 0, s, counts_dev, n, k, ids_dev,
                           n_ids_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    O3DMI_HIP_CHECK(hipMemcpyAsync(n_ids, n_ids_dev, sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

// float64 bounding box of n > 0 points; waits.
int o3dmi_internal_bounds(const void* points_dev, int64_t n, int dtype,
                          double* lo, double* hi, o3dmi_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    unsigned long long* box = nullptr;
    int st;
    if ((st = sc.Alloc(&box, 64))) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(box, 0xff, 24, s));
    O3DMI_HIP_CHECK(hipMemsetAsync(box + 3, 0, 24, s));
    const dim3 g(GridFor(n, kBlock, kCUs)), b(kBlock);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(BoundsKernel<double>, g, b, 0, s,
                           (const double*)points_dev, n, box);
    else
        hipLaunchKernelGGL(BoundsKernel<float>, g, b, 0, s,
                           (const float*)points_dev, n, box);
    O3DMI_HIP_CHECK(hipGetLastError());
    unsigned long long h[6];
    O3DMI_HIP_CHECK(hipMemcpyAsync(h, box, sizeof(h), hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    for (int a = 0; a < 3; ++a) {
        lo[a] = FromOrderedKey(h[a]);
        hi[a] = FromOrderedKey(h[3 + a]);
    }
    return O3DMI_OK;
}

int o3dmi_fpfh_from_neighbors(const void* points_dev, const void* normals_dev,
                              int64_t n_points, int dtype,
                              const int32_t* indices_dev,
                              const void* distance2_dev,
                              const int32_t* counts_dev,
                              const int64_t* row_splits_dev, int max_nn,
                              int64_t n_rows, const uint8_t* mask_dev,
                              const int64_t* map_info_idx_to_point_idx_dev,
                              void* fpfhs_dev, int64_t* n_fpfh_out,
                              o3dmi_stream_t stream) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(n_points >= 0 && n_points < (1ll << 31) && n_rows >= 0,
                  "size out of range");
    O3DMI_REQUIRE((mask_dev == nullptr) == (map_info_idx_to_point_idx_dev ==
                                            nullptr),
                  "Parameters mask and map_info_idx_to_point_idx must either "
                  "be both provided or both not provided.");
    O3DMI_REQUIRE((counts_dev == nullptr) != (row_splits_dev == nullptr),
                  "give counts (padded lists) or row_splits (CSR lists)");
    O3DMI_REQUIRE(!counts_dev || max_nn >= 1, "padded lists need max_nn >= 1");
    O3DMI_REQUIRE(mask_dev || n_rows == n_points,
                  "unfiltered lists must have one row per point");
    O3DMI_REQUIRE(n_rows == 0 || (indices_dev && distance2_dev),
                  "indices / distance2 are null");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    const Lists lists{indices_dev, counts_dev, row_splits_dev, max_nn};
    const size_t esz = dtype == O3DMI_F64 ? 8 : 4;
    int st;
    int32_t* fpfh_point = nullptr;
    int32_t* point_row = nullptr;
    int64_t n_out = n_points;
    if (mask_dev) {
        // NonZero(mask) and the inverse of map_info_idx_to_point_idx
        int32_t* m32 = nullptr;
        int64_t* pos = nullptr;
        void* tmp = nullptr;
        int* bad = nullptr;
        if ((st = sc.Alloc(&m32, 4 * (size_t)n_points)) ||
            (st = sc.Alloc(&pos, 8 * (size_t)(n_points + 1))) ||
            (st = sc.Alloc(&tmp, ScanScratchBytes(n_points))) ||
            (st = sc.Alloc(&fpfh_point, 4 * (size_t)n_points)) ||
            (st = sc.Alloc(&point_row, 4 * (size_t)n_points)) ||
            (st = sc.Alloc(&bad, sizeof(int))))
            return st;
        O3DMI_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), s));
        const dim3 g(GridFor(n_points, kBlock)), b(kBlock);
        if (n_points > 0) {
            hipLaunchKernelGGL(MaskToIntKernel, g, b, 0, s, mask_dev, n_points,
                               m32);
            if ((st = PrefixSumAsync(m32, n_points, false, pos, pos + n_points,
                                     tmp, s)))
                return st;
            hipLaunchKernelGGL(CompactKernel, g, b, 0, s, mask_dev, pos,
                               n_points, fpfh_point);
            hipLaunchKernelGGL(FillKernel, g, b, 0, s, point_row, n_points, -1);
        } else {
            O3DMI_HIP_CHECK(hipMemsetAsync(pos, 0, 8, s));
        }
        if (n_rows > 0)
            hipLaunchKernelGGL(InverseMapKernel, dim3(GridFor(n_rows, kBlock)),
                               b, 0, s, map_info_idx_to_point_idx_dev, n_rows,
                               n_points, point_row, bad);
        O3DMI_HIP_CHECK(hipMemcpyAsync(&n_out, pos + n_points, 8,
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        if (n_out > 0)
            hipLaunchKernelGGL(CheckRowsKernel, dim3(GridFor(n_out, kBlock,
                                                             1 << 30)),
                               b, 0, s, fpfh_point, n_out, point_row,
                               n_points, lists, bad);
        int hbad = 0;
        O3DMI_HIP_CHECK(hipMemcpyAsync(&hbad, bad, sizeof(int),
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        O3DMI_REQUIRE(!hbad,
                      "map_info_idx_to_point_idx must hold every masked point "
                      "and all of its neighbours");
    }
    if (n_fpfh_out) *n_fpfh_out = n_out;
    if (n_out == 0 && n_rows == 0) return O3DMI_OK;
    O3DMI_REQUIRE(points_dev && normals_dev && indices_dev && distance2_dev &&
                          fpfhs_dev,
                  "null argument");
    void* spfh = nullptr;
    if ((st = sc.Alloc(&spfh, esz * kFeat * (size_t)n_rows))) return st;
    const int64_t* row_point = mask_dev ? map_info_idx_to_point_idx_dev
                                        : nullptr;
    if (dtype == O3DMI_F64)
        return LaunchFpfh<double>(
                (const double*)points_dev, (const double*)normals_dev,
                (const double*)distance2_dev, lists, row_point, n_rows,
                fpfh_point, point_row, n_out, (double*)spfh,
                (double*)fpfhs_dev, s);
    return LaunchFpfh<float>((const float*)points_dev,
                             (const float*)normals_dev,
                             (const float*)distance2_dev, lists, row_point,
                             n_rows, fpfh_point, point_row, n_out,
                             (float*)spfh, (float*)fpfhs_dev, s);
}

// Internal (correspondence operator): nearest row of b for every row of a.
int o3dmi_internal_feature_nn1(const void* a_dev, int64_t na, const void* b_dev,
                               int64_t nb, int dim, int dtype,
                               int32_t* nn_dev, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "features must be Float32 or Float64");
    O3DMI_REQUIRE(dim >= 1, "feature dimension must be >= 1");
    O3DMI_REQUIRE(na >= 0 && na < (1ll << 31) && nb > 0 && nb < (1ll << 31),
                  "empty or oversized feature set");
    if (na == 0) return O3DMI_OK;
    O3DMI_REQUIRE(a_dev && b_dev && nn_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    // split the columns until there are ~4 workgroups per CU, keeping at
    // least 8 column tiles per slice
    const int64_t row_tiles = (na + kNnTile - 1) / kNnTile;
    const int64_t col_tiles = (nb + kNnTile - 1) / kNnTile;
    int64_t slices = (4 * kCUs + row_tiles - 1) / row_tiles;
    if (slices > col_tiles / 8) slices = col_tiles / 8;
    if (slices < 1) slices = 1;
    const int64_t cols = ((col_tiles + slices - 1) / slices) * kNnTile;
    slices = (nb + cols - 1) / cols;
    PoolScratch sc(s);
    double* pd = nullptr;
    int32_t* pi = nullptr;
    int st;
    if ((st = sc.Alloc(&pd, 8 * (size_t)(slices * na))) ||
        (st = sc.Alloc(&pi, 4 * (size_t)(slices * na))))
        return st;
    const dim3 grid((unsigned)row_tiles, (unsigned)slices), block(kNnBlock);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(Nn1Kernel<double>, grid, block, 0, s,
                           (const double*)a_dev, na, (const double*)b_dev, nb,
                           dim, cols, pd, pi);
    else
        hipLaunchKernelGGL(Nn1Kernel<float>, grid, block, 0, s,
                           (const float*)a_dev, na, (const float*)b_dev, nb,
                           dim, cols, pd, pi);
    hipLaunchKernelGGL(Nn1MergeKernel, dim3(GridFor(na, kBlock)), dim3(kBlock),
                       0, s, pd, pi, na, (int)slices, nn_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

// Internal (correspondence operator): the {K,2} int64 pairs of
// CorrespondencesFromFeatures from the 1-NN lists; info_dev[0] = K,
// info_dev[1] = fallback flag.
int o3dmi_internal_feature_mutual(const int32_t* ij_dev, const int32_t* ji_dev,
                                  int64_t n, int mutual_filter, float ratio,
                                  int64_t* corres_dev, int64_t* info_dev,
                                  o3dmi_stream_t stream) {
    O3DMI_REQUIRE(ij_dev && corres_dev && info_dev && n >= 0, "bad argument");
    O3DMI_REQUIRE(!mutual_filter || ji_dev, "ji is null");
    hipLaunchKernelGGL(MutualKernel, dim3(1), dim3(kMutualBlock), 0,
                       (hipStream_t)stream, ij_dev, ji_dev, n,
                       mutual_filter ? 1 : 0, ratio, corres_dev, info_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // extern "C"
