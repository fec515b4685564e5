// What the PointCloud operator families (filter, smooth, segment, sample)
// share on the device side: the attribute rows of a selection, the
// mask-and-count loop behind every elementwise mask, and the three launchers
// more than one family calls. Every launcher is stream-ordered and waits for
// nothing; masks are uint8 {n} holding 0 / 1.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "common.h"

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

// ---- mask and count ---------------------------------------------------------
// Adds the number of lanes with `keep` to *count: one atomic per wave. Every
// lane of the wave must call it.
__device__ __forceinline__ void CountKept(bool keep,
                                          unsigned long long* count) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
    if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(count, (unsigned long long)__popcll(m));
}

// Rounds of a grid-stride loop in which every lane takes part.
__device__ __forceinline__ int64_t Rounds(int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    return (n + stride - 1) / stride;
}

// mask[i] = keep_of(i) for i < n, and *count (zeroed by the caller) += the
// number of ones. keep_of is called for i < n only; every lane of every wave
// reaches CountKept in every round.
template <class Pred>
__device__ __forceinline__ void MaskAndCount(
        int64_t n, Pred keep_of, uint8_t* __restrict__ mask,
        unsigned long long* __restrict__ count) {
    const int64_t rounds = Rounds(n);
    for (int64_t r = 0; r < rounds; ++r) {
        const int64_t i = (r * gridDim.x + blockIdx.x) * (int64_t)blockDim.x +
                          threadIdx.x;
        bool keep = false;
        if (i < n) {
            keep = keep_of(i);
            mask[i] = keep ? 1 : 0;
        }
        CountKept(keep, count);
    }
}

// Pred: a small struct passed by value whose operator()(int64_t i) const is
// the predicate of row i.
template <class Pred>
__global__ void MaskKernel(int64_t n, Pred keep_of, uint8_t* __restrict__ mask,
                           unsigned long long* __restrict__ count) {
    MaskAndCount(n, keep_of, mask, count);
}

template <class Pred>
int LaunchMask(int64_t n, Pred keep_of, uint8_t* mask_dev,
               unsigned long long* count_dev, hipStream_t s) {
    hipLaunchKernelGGL(MaskKernel<Pred>, dim3(GridFor(n, kBlock)), dim3(kBlock),
                       0, s, n, keep_of, mask_dev, count_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

// ---- launchers more than one family calls -----------------------------------
// *bad_dev |= 1 when a coordinate is NaN or +-Inf (pointcloud_filter.hip).
int CheckFiniteAsync(const void* points_dev, int64_t n, int dtype,
                     int* bad_dev, hipStream_t s);
// mask[indices[r]] = 1 over a mask the caller has zeroed
// (pointcloud_filter.hip).
int IndexToMaskAsync(const int64_t* indices_dev, int64_t m, uint8_t* mask_dev,
                     hipStream_t s);
// *count_dev (zeroed by the caller) += the number of non-zero mask bytes
// (pointcloud_smooth.hip).
int CountMaskAsync(const uint8_t* mask_dev, int64_t n,
                   unsigned long long* count_dev, hipStream_t s);

}  // namespace o3dmi
