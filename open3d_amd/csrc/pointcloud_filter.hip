// Kernels behind PointCloud::SelectByMask / SelectByIndex and the Remove*
// filters (t/geometry/PointCloud.cpp:435-494, 650-760). The reference builds
// these from tensor ops (IndexGet, Sqrt, Mean, a HashSet insert); here each is
// one or two launches over the cloud:
//
//   compaction     flags -> PrefixSumAsync -> one scatter of up to 8 attributes;
//                  kept rows stay in input order (the scan decides the row, no
//                  atomics), so the result is the same on every run
//   non-finite     one pass
//   duplicates     rep_table.h: open-addressing table of point INDICES keyed by
//                  the bit pattern of the point (the block hash holds keys within
//                  +-2^20 only); equal keys meet in one slot and keep the
//                  lowest index with atomicMin, so the survivor of a key does
//                  not depend on which thread came first
//   radius         threshold on the counts of the fixed-radius count kernel
//   statistical    mean and centred sum of the per-point average distances
//                  (written by the KNN search through AvgDistanceOut below)
//                  as float64 sums in the fixed tree of reduce_sums.h, then the
//                  threshold and the mask in one launch
//
// All of it is HBM-bound streaming except the table inserts (one atomic per
// probe, load factor <= 1/2).

#include "pointcloud_filter.h"

#include "common.h"
#include "nns_wave.h"
#include "reduce_sums.h"
#include "rep_table.h"
#include "scan.h"

namespace o3dmi {
namespace {

// ---- compaction ---------------------------------------------------------------
__global__ void MaskFlagsKernel(const uint8_t* __restrict__ mask, int64_t n,
                                int invert, int32_t* __restrict__ flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        flags[i] = ((mask[i] != 0) != (invert != 0)) ? 1 : 0;
}

__global__ void CompactRowsKernel(const int32_t* __restrict__ flags,
                                  const long long* __restrict__ offsets,
                                  int64_t n, SelectAttrs a, unsigned words) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        if (flags[i]) MoveRow(a, words, i, offsets[i]);
}

__global__ void IndexRangeKernel(const int64_t* __restrict__ idx, int64_t m,
                                 int64_t n, int* __restrict__ bad) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < m;
         r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx[r];
        if (i < 0 || i >= n) atomicOr(bad, 1);
    }
}

__global__ void GatherRowsByIndexKernel(const int64_t* __restrict__ idx,
                                        int64_t m, SelectAttrs a,
                                        unsigned words) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < m;
         r += (int64_t)gridDim.x * blockDim.x)
        MoveRow(a, words, idx[r], r);
}

__global__ void IndexMaskKernel(const int64_t* __restrict__ idx, int64_t m,
                                uint8_t* __restrict__ mask) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < m;
         r += (int64_t)gridDim.x * blockDim.x)
        mask[idx[r]] = 1;  // every writer stores the same byte
}

// ---- non-finite -----------------------------------------------------------------
template <typename T>
__global__ void FiniteCheckKernel(const T* __restrict__ p, int64_t n3,
                                  int* __restrict__ bad) {
    bool any = false;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n3;
         i += (int64_t)gridDim.x * blockDim.x)
        any |= !isfinite(p[i]);
    if (any) atomicOr(bad, 1);
}

template <typename T>
struct NonFinitePred {
    const T* p;
    int remove_nan, remove_inf;
    __device__ __forceinline__ bool operator()(int64_t i) const {
        const T x = p[3 * i + 0], y = p[3 * i + 1], z = p[3 * i + 2];
        const bool has_nan = isnan(x) || isnan(y) || isnan(z);
        const bool has_inf = isinf(x) || isinf(y) || isinf(z);
        return !((remove_nan && has_nan) || (remove_inf && has_inf));
    }
};

// ---- duplicates -----------------------------------------------------------------
// The bit pattern of the point as the key of rep_table.h's table.
template <typename W>
struct PointBitKeys {
    using Word = W;
    const W* p;
    __device__ __forceinline__ int operator()(int64_t i, W k[3]) const {
        k[0] = p[3 * i + 0];
        k[1] = p[3 * i + 1];
        k[2] = p[3 * i + 2];
        return kKeyed;
    }
};

template <typename W>
struct DuplicatePred {
    PointBitKeys<W> keys;
    const int32_t* table;
    uint32_t slot_mask;
    __device__ __forceinline__ bool operator()(int64_t i) const {
        W k[3];
        keys(i, k);
        return RepFind(keys, i, k, table, slot_mask) == (int32_t)i;
    }
};

// ---- radius -----------------------------------------------------------------------
struct CountThresholdPred {
    const int32_t* counts;
    int nb_points;
    __device__ __forceinline__ bool operator()(int64_t i) const {
        return counts[i] >= nb_points;
    }
};

// ---- statistical ------------------------------------------------------------------
// AvgDistanceOut (KnnSearchKernel's output policy): only the mean distance to
// the neighbours
// (RemoveStatisticalOutliers: distance2.Sqrt().Mean({1}), t/geometry/
// PointCloud.cpp:700) -- no {q, knn} array exists on this path. The sum runs
// over the neighbours in list order (ascending by (d2, index)) in T and is
// divided by the row width in T, so the value does not depend on how the
// wave found the list.
template <typename T>
struct AvgDistanceOut {
    T* avg;
    __device__ __forceinline__ void Write(const WaveTopK<T>& list,
                                          int64_t i) const {
        T sum = T(0);
        for (int j = 0; j < list.nbest; ++j)
            sum += SqrtOf(__shfl(list.best_d, j));
        if ((threadIdx.x & 63) == 0) avg[i] = sum / (T)list.knn;
    }
};

// kCentred: sum of (avg_i - mean)^2 with mean = sum_in[0] / n, else sum of
// avg_i. One partial per workgroup; the geometry depends on n alone.
template <typename T, bool kCentred>
__global__ void __launch_bounds__(kSumsBlock)
AvgSumKernel(const T* __restrict__ avg, int64_t n,
             const double* __restrict__ sum_in, double* __restrict__ partials) {
    const double mean = kCentred ? sum_in[0] / (double)n : 0.0;
    double acc[1] = {0.0};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const double v = (double)avg[i];
        if (kCentred) {
            const double c = v - mean;
            acc[0] += c * c;
        } else {
            acc[0] += v;
        }
    }
    BlockSumAndStore<1>(acc, partials);
}

template <typename T>
__global__ void StatisticalMaskKernel(const T* __restrict__ avg, int64_t n,
                                      const double* __restrict__ sums,
                                      double std_ratio,
                                      double* __restrict__ stats,
                                      uint8_t* __restrict__ mask) {
    const double mean = sums[0] / (double)n;
    // n == 1: 0 / 0, the threshold is NaN and nothing is kept (as upstream)
    const double sd = sqrt(sums[1] / (double)(n - 1));
    const double threshold = mean + std_ratio * sd;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[0] = mean;
        stats[1] = sd;
        stats[2] = threshold;
    }
    MaskAndCount(
            n, [=](int64_t i) { return (double)avg[i] <= threshold; }, mask,
            (unsigned long long*)(stats + 3));
}

constexpr int64_t kMaskLimit = 1ll << 40;  // rows; keeps 3 * i in int64 by far

}  // namespace

size_t CompactScratchBytes(int64_t n) {
    const size_t rows = (size_t)(n > 0 ? n : 1);
    return sizeof(int64_t) * rows + ((sizeof(int32_t) * rows + 7) & ~(size_t)7) +
           ScanScratchBytes(n);
}

int CompactByMaskAsync(const uint8_t* mask_dev, int64_t n, bool invert,
                       const SelectAttrs& attrs, int64_t* count_dev,
                       void* scratch_dev, hipStream_t s) {
    if (n <= 0) {
        O3DMI_HIP_CHECK(hipMemsetAsync(count_dev, 0, sizeof(int64_t), s));
        return O3DMI_OK;
    }
    const size_t rows = (size_t)n;
    long long* offsets = (long long*)scratch_dev;
    int32_t* flags = (int32_t*)(offsets + rows);
    void* tiles = (char*)flags + ((sizeof(int32_t) * rows + 7) & ~(size_t)7);
    const dim3 grid(GridFor(n, kBlock)), block(kBlock);
    hipLaunchKernelGGL(MaskFlagsKernel, grid, block, 0, s, mask_dev, n,
                       invert ? 1 : 0, flags);
    const int st = PrefixSumAsync(flags, n, false, (int64_t*)offsets, count_dev,
                                  tiles, s);
    if (st) return st;
    hipLaunchKernelGGL(CompactRowsKernel, grid, block, 0, s, flags, offsets, n,
                       attrs, WordAttrs(attrs));
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int CheckIndexRangeAsync(const int64_t* indices_dev, int64_t m, int64_t n,
                         int* bad_dev, hipStream_t s) {
    if (m <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(IndexRangeKernel, dim3(GridFor(m, kBlock)), dim3(kBlock),
                       0, s, indices_dev, m, n, bad_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int GatherByIndexAsync(const int64_t* indices_dev, int64_t m,
                       const SelectAttrs& attrs, hipStream_t s) {
    if (m <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(GatherRowsByIndexKernel, dim3(GridFor(m, kBlock)),
                       dim3(kBlock), 0, s, indices_dev, m, attrs,
                       WordAttrs(attrs));
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int IndexToMaskAsync(const int64_t* indices_dev, int64_t m, uint8_t* mask_dev,
                     hipStream_t s) {
    if (m <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(IndexMaskKernel, dim3(GridFor(m, kBlock)), dim3(kBlock),
                       0, s, indices_dev, m, mask_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int CheckFiniteAsync(const void* points_dev, int64_t n, int dtype,
                     int* bad_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    O3DMI_REQUIRE(n < kMaskLimit, "too many points");
    const dim3 grid(GridFor(3 * n, kBlock)), block(kBlock);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(FiniteCheckKernel<double>, grid, block, 0, s,
                           (const double*)points_dev, 3 * n, bad_dev);
    else
        hipLaunchKernelGGL(FiniteCheckKernel<float>, grid, block, 0, s,
                           (const float*)points_dev, 3 * n, bad_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int NonFiniteMaskAsync(const void* points_dev, int64_t n, int dtype,
                       bool remove_nan, bool remove_inf, uint8_t* mask_dev,
                       unsigned long long* count_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    O3DMI_REQUIRE(n < kMaskLimit, "too many points");
    const int no_nan = remove_nan ? 1 : 0, no_inf = remove_inf ? 1 : 0;
    return dtype == O3DMI_F64
                   ? LaunchMask(n,
                                NonFinitePred<double>{(const double*)points_dev,
                                                      no_nan, no_inf},
                                mask_dev, count_dev, s)
                   : LaunchMask(n,
                                NonFinitePred<float>{(const float*)points_dev,
                                                     no_nan, no_inf},
                                mask_dev, count_dev, s);
}

int64_t DuplicateTableSlots(int64_t n) {
    int64_t slots = 64;
    while (slots < 2 * n) slots <<= 1;
    return slots;
}

int DuplicateMaskAsync(const void* points_dev, int64_t n, int dtype,
                       int32_t* table_dev, int64_t slots, uint8_t* mask_dev,
                       unsigned long long* count_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    // the table holds int32 indices and is addressed by 32-bit slot numbers
    O3DMI_REQUIRE(n < (1ll << 30), "too many points (< 2^30)");
    O3DMI_REQUIRE(slots >= 2 * n && (slots & (slots - 1)) == 0,
                  "duplicate table: bad capacity");
    O3DMI_HIP_CHECK(hipMemsetAsync(table_dev, 0xFF,
                                   sizeof(int32_t) * (size_t)slots, s));
    const dim3 grid(GridFor(n, kBlock)), block(kBlock);
    const uint32_t slot_mask = (uint32_t)(slots - 1);
    if (dtype == O3DMI_F64) {
        const PointBitKeys<uint64_t> keys = {(const uint64_t*)points_dev};
        hipLaunchKernelGGL(RepInsertKernel<PointBitKeys<uint64_t>>, grid,
                           block, 0, s, keys, n, table_dev, slot_mask);
        return LaunchMask(n,
                          DuplicatePred<uint64_t>{keys, table_dev, slot_mask},
                          mask_dev, count_dev, s);
    }
    const PointBitKeys<uint32_t> keys = {(const uint32_t*)points_dev};
    hipLaunchKernelGGL(RepInsertKernel<PointBitKeys<uint32_t>>, grid, block, 0,
                       s, keys, n, table_dev, slot_mask);
    return LaunchMask(n, DuplicatePred<uint32_t>{keys, table_dev, slot_mask},
                      mask_dev, count_dev, s);
}

int CountThresholdMaskAsync(const int32_t* counts_dev, int64_t n,
                            int nb_points, uint8_t* mask_dev,
                            unsigned long long* count_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    return LaunchMask(n, CountThresholdPred{counts_dev, nb_points}, mask_dev,
                      count_dev, s);
}

size_t StatisticalScratchDoubles() { return (size_t)kSumsMaxGrid + 8; }

int StatisticalMaskAsync(const void* avg_dev, int64_t n, int dtype,
                         double std_ratio, double* scratch_dev,
                         double* stats_dev, uint8_t* mask_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    double* partials = scratch_dev;
    double* sums = scratch_dev + kSumsMaxGrid;  // {sum avg, centred sum}
    const int rows = SumsGrid(n);
    const dim3 grid(GridFor(n, kBlock)), block(kBlock);
#define O3DMI_STAT(T)                                                          \
    do {                                                                       \
        hipLaunchKernelGGL((AvgSumKernel<T, false>), dim3(rows),               \
                           dim3(kSumsBlock), 0, s, (const T*)avg_dev, n,       \
                           (const double*)nullptr, partials);                  \
        hipLaunchKernelGGL(FinalSumKernel<1>, dim3(1), dim3(kFinalThreads), 0, \
                           s, partials, rows, sums, (double*)nullptr,          \
                           (int*)nullptr, 0);                                  \
        hipLaunchKernelGGL((AvgSumKernel<T, true>), dim3(rows),                \
                           dim3(kSumsBlock), 0, s, (const T*)avg_dev, n, sums, \
                           partials);                                          \
        hipLaunchKernelGGL(FinalSumKernel<1>, dim3(1), dim3(kFinalThreads), 0, \
                           s, partials, rows, sums + 1, (double*)nullptr,      \
                           (int*)nullptr, 0);                                  \
        hipLaunchKernelGGL(StatisticalMaskKernel<T>, grid, block, 0, s,        \
                           (const T*)avg_dev, n, sums, std_ratio, stats_dev,   \
                           mask_dev);                                          \
    } while (0)
    if (dtype == O3DMI_F64) O3DMI_STAT(double);
    else O3DMI_STAT(float);
#undef O3DMI_STAT
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace o3dmi

// Internal (RemoveStatisticalOutliers): avg_dev[i] = mean over the
// min(knn, n) nearest points of point i (itself included, at distance 0) of
// sqrt(d2), in the point dtype; see AvgDistanceOut. Returns with the search
// queued on the stream (its scratch is released after a wait).
extern "C" int o3dmi_internal_nns_knn_avg_distance(const void* points_dev,
                                                   int64_t n, int dtype,
                                                   int knn, void* avg_dev,
                                                   o3dmi_stream_t stream) {
    using namespace o3dmi;
    O3DMI_REQUIRE(avg_dev != nullptr, "null argument");
    return KnnSearchRun(
            points_dev, n, points_dev, n, dtype, knn,
            [=](auto t) {
                using T = decltype(t);
                return AvgDistanceOut<T>{(T*)avg_dev};
            },
            (hipStream_t)stream);
}
