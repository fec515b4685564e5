// Private seam between pointcloud_sample.hip (kernels and their launchers) and
// host/pointcloud_sample.cpp (the C ABI of PointCloud::UniformDownSample /
// RandomDownSample / FarthestPointDownSample / Crop and the bounds). Every
// launcher is stream-ordered and waits for nothing; masks are uint8 {n}
// holding 0 / 1.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pointcloud_rows.h"

namespace o3dmi {

// ---- farthest-point order ---------------------------------------------------
// order[0] = start; order[i + 1] = the lowest index among the maxima of
// dist_j = min over i' <= i of |p_j - p_order[i']|^2, the square as
// ((dx dx) + dy dy) + dz dz in the point dtype. (max value, min index) is
// associative and commutative, so both forms give the same bits.

// Points one workgroup holds in registers (resident form), per dtype.
int64_t FarthestResidentCapacity(int dtype);
// One launch for all k samples; n <= FarthestResidentCapacity(dtype).
int FarthestOrderResidentAsync(const void* points_dev, int64_t n, int dtype,
                               int64_t k, int64_t start, int64_t* order_dev,
                               hipStream_t s);

// Scratch of the streamed form: dist {n} in the point dtype, one (value, index)
// partial per workgroup, the chosen index and the ticket.
size_t FarthestStreamScratchBytes(int64_t n, int dtype);
// Workgroups of the streamed form and the points in each one's slice; every
// workgroup has at least one point.
int FarthestStreamGrid(int64_t n, int64_t* slice_out);
// k - 1 launches enqueued back to back (and one that sets the words up).
int FarthestOrderStreamedAsync(const void* points_dev, int64_t n, int dtype,
                               int64_t k, int64_t start, int64_t* order_dev,
                               void* scratch_dev, hipStream_t s);

// ---- uniform / random -------------------------------------------------------
// out row i = in row i * every_k for i < m.
int StridedRowsAsync(int64_t m, int64_t every_k, const SelectAttrs& attrs,
                     hipStream_t s);
// indices[j] = SampleIndex(seed, n, j) for j < m.
int SampleIndicesAsync(uint64_t seed, int64_t n, int64_t m,
                       int64_t* indices_dev, hipStream_t s);

// ---- crop and bounds --------------------------------------------------------
// The boxes arrive as doubles and are rounded to the point dtype here.
// *count_dev (zeroed by the caller) receives the number of ones.
int AabbMaskAsync(const void* points_dev, int64_t n, int dtype,
                  const double min_bound[3], const double max_bound[3],
                  uint8_t* mask_dev, unsigned long long* count_dev,
                  hipStream_t s);
int ObbMaskAsync(const void* points_dev, int64_t n, int dtype,
                 const double center[3], const double rotation[9],
                 const double extent[3], uint8_t* mask_dev,
                 unsigned long long* count_dev, hipStream_t s);

// Scratch doubles of MinMaxBoundAsync (partial rows + the result).
size_t MinMaxScratchDoubles();
// result_dev: {min x, y, z, max x, y, z} as float64 (exact widenings). A NaN
// coordinate never wins a comparison and is skipped.
int MinMaxBoundAsync(const void* points_dev, int64_t n, int dtype,
                     double* scratch_dev, double** result_dev, hipStream_t s);

}  // namespace o3dmi
