// PointCloud::ComputeMetrics / ComputePointCloudDistance on the device
// (t/geometry/PointCloud.cpp:1805-1836, t/geometry/kernel/Metrics.cpp,
// geometry/PointCloud.cpp:133-157; upstream copies device clouds to the host
// and searches two k-d trees there).
//
// 1. NearestGroupKernel: the exact nearest target point of every query on the
//    finest level of the KNN index (nns.h), a group of kNearestGroup lanes per
//    query. It is the first pass of NearestSearchRun (KnnSearchRun of
//    nns_wave.h with knn = 1); what it cannot finish goes to the second pass
//    (KnnSearchKernel with NearestOut).
// 2. MetricsElementKernel / RunSumKernel: sqrt, the fixed-tree float64 sum,
//    the maximum and the F-score counts of the {q} distances.
#include "pointcloud_metrics.h"

#include "nns_wave.h"

namespace o3dmi {
namespace {

constexpr int kNearestBlock = 256;
constexpr int kNoNearest = 0x7fffffff;

// (d, i) = the lexicographic minimum of (d, i) and (od, oi).
template <typename T>
__device__ __forceinline__ void TakeLower(T& d, int& i, T od, int oi) {
    if (od < d || (od == d && oi < i)) {
        d = od;
        i = oi;
    }
}

// One step of a query's walk: the cells of the box [x0, x1] x [y0, y1] x
// [z0, z1] whose Chebyshev distance from the query's cell is >= r_skip, split
// over the lanes of the group; every record of a cell's bucket is compared.
// A bucket may hold records of other cells as well (the hash folds cells): they
// are points of the cloud like any other, and a minimum does not mind seeing a
// point twice. The three loop bounds (cells, records) are fixed before each
// loop starts.
template <typename T>
__device__ __forceinline__ void ScanBox(const NnsView<T>& nv, const T* qq,
                                        const long long* c, long long x0,
                                        long long x1, long long y0,
                                        long long y1, long long z0,
                                        long long z1, long long r_skip, int sub,
                                        T& best_d, int& best_i) {
    if (x1 < x0 || y1 < y0 || z1 < z0) return;
    const int nx = (int)(x1 - x0 + 1), ny = (int)(y1 - y0 + 1),
              nz = (int)(z1 - z0 + 1);
    const int n_cells = nx * ny * nz;
    for (int cell = sub; cell < n_cells; cell += kNearestGroup) {
        const int ix = cell % nx, iy = (cell / nx) % ny, iz = cell / (nx * ny);
        const long long x = x0 + ix, y = y0 + iy, z = z0 + iz;
        long long ax = x - c[0], ay = y - c[1], az = z - c[2];
        ax = ax < 0 ? -ax : ax;
        ay = ay < 0 ? -ay : ay;
        az = az < 0 ? -az : az;
        if (max(ax, max(ay, az)) < r_skip) continue;  // seen in an earlier step
        unsigned s0, e0;
        BucketRange(nv, HashCell(x, y, z) & nv.mask, s0, e0);
        for (unsigned j = s0; j < e0; ++j) {
            const Rec4<T> p = nv.sorted[j];
            T result = T(0);
            const T d0 = qq[0] - p.x;
            result += d0 * d0;
            const T d1 = qq[1] - p.y;
            result += d1 * d1;
            const T dd = qq[2] - p.z;
            result += dd * dd;
            TakeLower(best_d, best_i, result, RecIndex(p));
        }
    }
}

// Exact 1-NN on one level. The walk and its stop rule are KnnSearchKernel's for
// knn = 1: the cube of radius max(r0, first_radius) first, then one shell at a
// time up to kKnnShells, all clipped to the occupied box; after shell r every
// unvisited point is at least r cell + margin away, so the query is finished
// once its best d2 is below that bound squared (less 1e-6), or once the cube
// covers the box. Every lane of a wave runs the same kKnnShells + 1 steps at
// most and joins every shuffle; a group that has finished scans nothing.
template <typename T>
__global__ void __launch_bounds__(kNearestBlock)
NearestGroupKernel(KnnGrid<T> g, const T* __restrict__ q, int64_t nq,
                   int first_radius, int exhaustive, int* __restrict__ retry_ids,
                   int* __restrict__ retry_count, T* __restrict__ d2_out,
                   int* __restrict__ idx_out) {
    constexpr int G = kNearestGroup;
    const int lane = threadIdx.x & 63;
    const int sub = lane & (G - 1);
    const int64_t n_groups = ((int64_t)gridDim.x * blockDim.x) / G;
    // first group of this wave: the trip count is the same in all its lanes
    const int64_t wave_group =
            (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * (64 / G);
    for (int64_t base = wave_group; base < nq; base += n_groups) {
        const int64_t i = base + lane / G;
        const bool valid = i < nq;
        const int64_t ic = valid ? i : nq - 1;
        const T qq[3] = {q[3 * ic + 0], q[3 * ic + 1], q[3 * ic + 2]};
        long long c[3];
        CellOf(qq, g.nv.inv_cell, c[0], c[1], c[2]);
        // distance to the nearest face of the query's own cell
        double margin = g.cell;
        long long r0 = 0, rmax = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double lo = (double)qq[a] - (double)c[a] * g.cell;
            const double hi = (double)(c[a] + 1) * g.cell - (double)qq[a];
            margin = fmin(margin, fmin(lo, hi));
            const long long below = g.cmin[a] - c[a];
            const long long above = c[a] - g.cmax[a];
            r0 = max(r0, max(below, above));        // shells before the box
            rmax = max(rmax, max(-below, -above));  // shell covering the box
        }
        // cell assignment rounds in float64: keep a small absolute slack
        margin -= 1e-7 * g.cell;
        if (!(margin > 0)) margin = 0;

        T best_d = (T)INFINITY;
        int best_i = kNoNearest;
        bool done = false;
        long long r = r0 > first_radius ? r0 : first_radius;
        // out of reach of this level: nothing to scan, left to the second pass
        bool open = valid && (exhaustive || r0 <= kKnnShells);
        bool first = true;
        for (int step = 0; step <= kKnnShells; ++step) {
            const bool active = open && !done && (exhaustive ? step == 0
                                                             : r <= kKnnShells);
            if (!__any(active)) break;
            if (active) {
                if (exhaustive)
                    ScanBox(g.nv, qq, c, g.cmin[0], g.cmax[0], g.cmin[1],
                            g.cmax[1], g.cmin[2], g.cmax[2], 0, sub, best_d,
                            best_i);
                else
                    ScanBox(g.nv, qq, c, max(c[0] - r, g.cmin[0]),
                            min(c[0] + r, g.cmax[0]), max(c[1] - r, g.cmin[1]),
                            min(c[1] + r, g.cmax[1]), max(c[2] - r, g.cmin[2]),
                            min(c[2] + r, g.cmax[2]), first ? 0 : r, sub,
                            best_d, best_i);
            }
            // minimum by (d2, index) over the G lanes of the group
#pragma unroll
            for (int m = 1; m < G; m <<= 1) {
                const T od = __shfl_xor(best_d, m, G);
                const int oi = __shfl_xor(best_i, m, G);
                TakeLower(best_d, best_i, od, oi);
            }
            if (active) {
                if (exhaustive) {
                    done = true;
                } else {
                    const double bound = (double)r * g.cell + margin;
                    if (best_i != kNoNearest &&
                        (double)best_d < bound * bound * (1.0 - 1e-6))
                        done = true;
                    else if (r >= rmax)  // nothing of the box lies beyond
                        done = true;
                    first = false;
                    ++r;
                }
            }
        }
        if (valid && sub == 0) {
            if (done) {
                d2_out[i] = best_d;
                if (idx_out) idx_out[i] = best_i;
            } else if (retry_ids) {
                retry_ids[atomicAdd(retry_count, 1)] = (int)i;
            }
        }
    }
}

// ---- the reduction ----------------------------------------------------------
constexpr int kReduceBlock = 256;
constexpr int kReduceRuns = 8;  // runs of kMetricsRun values per workgroup

struct Radii {
    float r[kMetricsRadiusGroup];
    int n;
};

// grid = ceil(q / (kReduceRuns kMetricsRun)). dist_out may be d2 itself: a
// thread reads its own element before it writes it.
template <typename T, bool SUM>
__global__ void __launch_bounds__(kReduceBlock)
MetricsElementKernel(const T* d2, int64_t q, T* dist_out, Radii radii,
                     MetricsWords* __restrict__ words,
                     double* __restrict__ run_sums) {
    constexpr int kTile = kReduceRuns * kMetricsRun;
    __shared__ T tile[SUM ? kTile : 1];
    const int64_t base = (int64_t)blockIdx.x * kTile;
    T mx = T(0);
    unsigned cnt[kMetricsRadiusGroup];
#pragma unroll
    for (int k = 0; k < kMetricsRadiusGroup; ++k) cnt[k] = 0;
    for (int e = threadIdx.x; e < kTile; e += kReduceBlock) {
        const int64_t i = base + e;
        if (i >= q) break;
        const T d = SqrtOf(d2[i]);
        if (dist_out) dist_out[i] = d;
        if (SUM) {
            tile[e] = d;
            mx = d > mx ? d : mx;
        }
#pragma unroll
        for (int k = 0; k < kMetricsRadiusGroup; ++k)
            if (k < radii.n && d < (T)radii.r[k]) ++cnt[k];
    }
    // counts and the maximum are order-free: wave, then one atomic per wave
#pragma unroll
    for (int k = 0; k < kMetricsRadiusGroup; ++k) {
        if (k >= radii.n) break;
        unsigned v = cnt[k];
        for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
        if ((threadIdx.x & 63) == 0 && v)
            atomicAdd(&words->counts[k], (unsigned long long)v);
    }
    if (!SUM) return;
    for (int m = 32; m > 0; m >>= 1) {
        const T o = __shfl_xor(mx, m);
        mx = o > mx ? o : mx;
    }
    // d >= 0: the bits of the widened value order like the value
    if ((threadIdx.x & 63) == 0)
        atomicMax(&words->max_bits,
                  (unsigned long long)__double_as_longlong((double)mx));
    __syncthreads();
    if (threadIdx.x < kReduceRuns) {
        const int64_t run = (int64_t)blockIdx.x * kReduceRuns + threadIdx.x;
        const int64_t start = run * kMetricsRun;
        if (start < q) {
            const int len = (int)(q - start < kMetricsRun ? q - start
                                                          : kMetricsRun);
            const T* v = tile + threadIdx.x * kMetricsRun;
            double sum = (double)v[0];
            for (int j = 1; j < len; ++j) sum += (double)v[j];
            run_sums[run] = sum;
        }
    }
}

// out[r] = the values in[512 r ..] added in index order; one thread per run.
__global__ void RunSumKernel(const double* __restrict__ in, int64_t m,
                             double* __restrict__ out) {
    const int64_t run = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t start = run * kMetricsRun;
    if (start >= m) return;
    const int len = (int)(m - start < kMetricsRun ? m - start : kMetricsRun);
    double sum = in[start];
#pragma unroll 8  // the loads do not depend on the adds: eight in flight
    for (int j = 1; j < len; ++j) sum += in[start + j];
    out[run] = sum;
}

inline int64_t RunsOf(int64_t m) {
    return (m + kMetricsRun - 1) / kMetricsRun;
}

template <typename T>
int LaunchReduce(const void* d2_dev, int64_t q, void* dist_out_dev,
                 const Radii& radii, bool sum_and_max, MetricsWords* words_dev,
                 double* sums_dev, hipStream_t s) {
    const int64_t tile = (int64_t)kReduceRuns * kMetricsRun;
    const dim3 grid((unsigned)((q + tile - 1) / tile)), block(kReduceBlock);
    if (sum_and_max)
        hipLaunchKernelGGL((MetricsElementKernel<T, true>), grid, block, 0, s,
                           (const T*)d2_dev, q, (T*)dist_out_dev, radii,
                           words_dev, sums_dev);
    else
        hipLaunchKernelGGL((MetricsElementKernel<T, false>), grid, block, 0, s,
                           (const T*)d2_dev, q, (T*)dist_out_dev, radii,
                           words_dev, sums_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

// NearestOut: the second pass of NearestSearchRun (knn = 1): the squared
// distance to the nearest point into slot i and, when asked, its index.
template <typename T>
struct NearestOut {
    T* d2;
    int* idx;
    __device__ __forceinline__ void Write(const WaveTopK<T>& list,
                                          int64_t i) const {
        if ((threadIdx.x & 63) == 0) {
            d2[i] = list.best_d;
            if (idx) idx[i] = list.best_i;
        }
    }
};

// The first pass over all q queries: a group of kNearestGroup lanes walks the
// finest level's growing cubes for a query and either writes its slot of
// d2_dev / idx_dev or appends the query to the retry list.
int NearestFirstPassAsync(const KnnFirstPass& fp, int dtype,
                          const void* queries_dev, int64_t q, void* d2_dev,
                          int32_t* idx_dev, hipStream_t s) {
    const dim3 grid(GridFor(q, kNearestBlock / kNearestGroup, kCUs * 16)),
            block(kNearestBlock);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(NearestGroupKernel<double>, grid, block, 0, s,
                           MakeKnnGrid<double>(fp.finest, fp.cmin, fp.cmax),
                           (const double*)queries_dev, q, fp.first_radius,
                           fp.exhaustive, fp.retry_ids, fp.retry_count,
                           (double*)d2_dev, idx_dev);
    else
        hipLaunchKernelGGL(NearestGroupKernel<float>, grid, block, 0, s,
                           MakeKnnGrid<float>(fp.finest, fp.cmin, fp.cmax),
                           (const float*)queries_dev, q, fp.first_radius,
                           fp.exhaustive, fp.retry_ids, fp.retry_count,
                           (float*)d2_dev, idx_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace

int NearestSearchRun(const void* points_dev, int64_t n, const void* queries_dev,
                     int64_t q, int dtype, void* d2_dev, int32_t* idx_dev,
                     int64_t* second_pass_queries, hipStream_t s) {
    // (a missing d2_dev is reported where a missing queries_dev is: after the
    // size checks, as "null argument")
    return KnnSearchRun(
            points_dev, n, d2_dev ? queries_dev : nullptr, q, dtype, 1,
            [=](auto t) {
                using T = decltype(t);
                return NearestOut<T>{(T*)d2_dev, idx_dev};
            },
            s,
            [=](const KnnFirstPass& fp) {
                return NearestFirstPassAsync(fp, dtype, queries_dev, q, d2_dev,
                                             idx_dev, s);
            },
            second_pass_queries);
}

size_t MetricsSumScratchDoubles(int64_t q) {
    int64_t m = RunsOf(q > 0 ? q : 1);
    size_t total = (size_t)m;
    while (m > 1) {
        m = RunsOf(m);
        total += (size_t)m;
    }
    return total;
}

int MetricsReduceAsync(const void* d2_dev, int64_t q, int dtype,
                       void* dist_out_dev, const float* radii, int n_radii,
                       bool sum_and_max, MetricsWords* words_dev,
                       double* sums_dev, const double** total_dev,
                       hipStream_t s) {
    O3DMI_REQUIRE(d2_dev && q > 0 && words_dev, "null argument");
    O3DMI_REQUIRE(n_radii >= 0 && n_radii <= kMetricsRadiusGroup &&
                          (n_radii == 0 || radii),
                  "metrics: radius group out of range");
    O3DMI_REQUIRE(!sum_and_max || (sums_dev && total_dev), "null argument");
    Radii group;
    group.n = n_radii;
    for (int k = 0; k < kMetricsRadiusGroup; ++k)
        group.r[k] = k < n_radii ? radii[k] : 0.0f;
    int st = dtype == O3DMI_F64
                     ? LaunchReduce<double>(d2_dev, q, dist_out_dev, group,
                                            sum_and_max, words_dev, sums_dev, s)
                     : LaunchReduce<float>(d2_dev, q, dist_out_dev, group,
                                           sum_and_max, words_dev, sums_dev, s);
    if (st || !sum_and_max) return st;
    double* level = sums_dev;
    int64_t m = RunsOf(q);
    while (m > 1) {
        const int64_t runs = RunsOf(m);
        hipLaunchKernelGGL(RunSumKernel, dim3(GridFor(runs, 64)), dim3(64), 0,
                           s, level, m, level + m);
        level += m;
        m = runs;
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    *total_dev = level;
    return O3DMI_OK;
}

}  // namespace o3dmi
