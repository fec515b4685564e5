// Private seam between pointcloud_filter.hip (kernels and their launchers) and
// host/pointcloud_filter.cpp (the C ABI of PointCloud::SelectByMask /
// SelectByIndex / Remove*Outliers / RemoveNonFinitePoints /
// RemoveDuplicatedPoints). Every launcher is stream-ordered and waits for
// nothing; masks are uint8 {n} holding 0 / 1.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace o3dmi {

constexpr int kMaxSelectAttrs = 8;

// Up to eight attributes of one cloud, moved row by row in the same launch.
struct SelectAttrs {
    const void* in[kMaxSelectAttrs];
    void* out[kMaxSelectAttrs];
    long long row_bytes[kMaxSelectAttrs];
    int n_attrs;
};

// Row `src` of every attribute to row `dst`. words: bit a set = attribute a is
// 4-byte aligned with a width that is a multiple of 4 (positions, normals,
// float colours); the others (uint8 colours) move byte by byte.
__device__ __forceinline__ void MoveRow(const SelectAttrs& a, unsigned words,
                                        int64_t src, int64_t dst) {
    for (int k = 0; k < a.n_attrs; ++k) {
        const long long w = a.row_bytes[k];
        if (words & (1u << k)) {
            const uint32_t* in = (const uint32_t*)a.in[k] + src * (w >> 2);
            uint32_t* out = (uint32_t*)a.out[k] + dst * (w >> 2);
            if (w == 12) {
                const uint32_t x = in[0], y = in[1], z = in[2];
                out[0] = x;
                out[1] = y;
                out[2] = z;
            } else {
                for (long long b = 0; b < (w >> 2); ++b) out[b] = in[b];
            }
        } else {
            const uint8_t* in = (const uint8_t*)a.in[k] + src * w;
            uint8_t* out = (uint8_t*)a.out[k] + dst * w;
            for (long long b = 0; b < w; ++b) out[b] = in[b];
        }
    }
}

// The `words` mask of MoveRow for these attributes.
inline unsigned WordAttrs(const SelectAttrs& a) {
    unsigned words = 0;
    for (int k = 0; k < a.n_attrs; ++k)
        if (((uintptr_t)a.in[k] | (uintptr_t)a.out[k] |
             (uintptr_t)a.row_bytes[k]) % 4 == 0)
            words |= 1u << k;
    return words;
}

// Scratch of CompactByMaskAsync: int32 flags {n}, int64 offsets {n}, the
// scan's tile totals.
size_t CompactScratchBytes(int64_t n);

// Stable compaction: row i of every attribute goes to row (number of kept rows
// before i) when (mask[i] != 0) != invert. *count_dev receives the number of
// kept rows.
int CompactByMaskAsync(const uint8_t* mask_dev, int64_t n, bool invert,
                       const SelectAttrs& attrs, int64_t* count_dev,
                       void* scratch_dev, hipStream_t s);

// *bad_dev |= 1 when an index lies outside [0, n). Writes nothing else.
int CheckIndexRangeAsync(const int64_t* indices_dev, int64_t m, int64_t n,
                         int* bad_dev, hipStream_t s);
// out row r = in row indices[r] (indices already checked).
int GatherByIndexAsync(const int64_t* indices_dev, int64_t m,
                       const SelectAttrs& attrs, hipStream_t s);
// mask[indices[r]] = 1 over a mask the caller has zeroed.
int IndexToMaskAsync(const int64_t* indices_dev, int64_t m, uint8_t* mask_dev,
                     hipStream_t s);

// *bad_dev |= 1 when a coordinate is NaN or +-Inf.
int CheckFiniteAsync(const void* points_dev, int64_t n, int dtype,
                     int* bad_dev, hipStream_t s);
// The three remove_nan / remove_inf forms; *count_dev (zeroed by the caller)
// receives the number of ones.
int NonFiniteMaskAsync(const void* points_dev, int64_t n, int dtype,
                       bool remove_nan, bool remove_inf, uint8_t* mask_dev,
                       unsigned long long* count_dev, hipStream_t s);

// Open-addressing table of point indices keyed by the bit pattern of the
// point; capacity a power of two >= 2 n.
int64_t DuplicateTableSlots(int64_t n);
int DuplicateMaskAsync(const void* points_dev, int64_t n, int dtype,
                       int32_t* table_dev, int64_t slots, uint8_t* mask_dev,
                       unsigned long long* count_dev, hipStream_t s);

// mask_i = counts_i >= nb_points.
int CountThresholdMaskAsync(const int32_t* counts_dev, int64_t n,
                            int nb_points, uint8_t* mask_dev,
                            unsigned long long* count_dev, hipStream_t s);

// Scratch doubles of StatisticalMaskAsync (partial rows + the two sums).
size_t StatisticalScratchDoubles();
// avg {n} in the point dtype -> mean, sample standard deviation, threshold
// (float64, fixed summation tree) and mask_i = (double)avg_i <= threshold.
// stats_dev: {mean, std, threshold} as doubles, then the survivor count as a
// 64-bit integer (32 bytes in all, zeroed by the caller).
int StatisticalMaskAsync(const void* avg_dev, int64_t n, int dtype,
                         double std_ratio, double* scratch_dev,
                         double* stats_dev, uint8_t* mask_dev, hipStream_t s);

}  // namespace o3dmi
