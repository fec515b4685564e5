// Device pieces shared by the rigid (slac.hip) and non-rigid
// (slac_nonrigid.hip) alignment kernels: the float32 row arithmetic of a pose,
// the 29 pose terms of one pair and the fixed-order sum of partial rows.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "slac.h"

namespace o3dmi {

// r, threshold test and the 29 terms of one pair from the transformed
// p' = Ti p, q' = Tj q, n' = Ri n (kernel/FillInLinearSystemImpl.h:27-38,
// 95-112). `take` false adds zeros.
__device__ __forceinline__ void AccumulateRigidPair(
        double (&A)[kSlacSums], bool take, float px, float py, float pz,
        float qx, float qy, float qz, float nx, float ny, float nz,
        float threshold) {
    const float r = (px - qx) * nx + (py - qy) * ny + (pz - qz) * nz;
    take = take && !(fabsf(r) > threshold);
    const float J[6] = {-qz * ny + qy * nz, qz * nx - qx * nz,
                        -qy * nx + qx * ny, nx, ny, nz};
    int s = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int k = 0; k <= j; ++k) {
            const float v = J[j] * J[k];
            A[s++] += take ? (double)v : 0.0;
        }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float v = J[k] * r;
        A[21 + k] += take ? (double)v : 0.0;
    }
    const float rr = r * r;
    A[27] += take ? (double)rr : 0.0;
    A[28] += take ? 1.0 : 0.0;
}

// TransformPointsKernel's row: t0 x + t1 y + t2 z + t3.
__device__ __forceinline__ float Row(const float* t, float x, float y,
                                     float z) {
    return t[0] * x + t[1] * y + t[2] * z + t[3];
}
__device__ __forceinline__ float RotRow(const float* t, float x, float y,
                                        float z) {
    return t[0] * x + t[1] * y + t[2] * z;
}

// Rows [first, last) of the partials added in a fixed order by one workgroup
// of kSlacBlock lanes: lane (rl, col) = (tid / 32, tid % 32) strides over the
// rows, the 8 row-lanes are then added in order. The totals are in
// lds[0][0..28] afterwards (all lanes may read them).
__device__ __forceinline__ void SumRows(const double* __restrict__ partials,
                                        int64_t first, int64_t last,
                                        double (&lds)[kSlacBlock / 32][32]) {
    const int col = threadIdx.x & 31;
    const int rl = threadIdx.x >> 5;
    double v = 0;
    if (col < kSlacSums)
        for (int64_t r = first + rl; r < last; r += kSlacBlock / 32)
            v += partials[r * kSlacSums + col];
    lds[rl][col] = v;
    __syncthreads();
    if (threadIdx.x < 32) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < kSlacBlock / 32; ++k) s += lds[k][threadIdx.x];
        lds[0][threadIdx.x] = s;
    }
    __syncthreads();
}

}  // namespace o3dmi
