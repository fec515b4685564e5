// Private seam between pointcloud_filter.hip (kernels and their launchers) and
// host/pointcloud_filter.cpp (the C ABI of PointCloud::SelectByMask /
// SelectByIndex / Remove*Outliers / RemoveNonFinitePoints /
// RemoveDuplicatedPoints). Every launcher is stream-ordered and waits for
// nothing; masks are uint8 {n} holding 0 / 1.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pointcloud_rows.h"

namespace o3dmi {

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
