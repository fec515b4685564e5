// Device helpers of slac::ControlGrid shared by control_grid.hip and
// slac_nonrigid.hip: the cell of a point, its eight corner nodes, the
// trilinear ratios and the corner-order interpolation. float32 in the
// reference's operation order (t/pipelines/slac/ControlGrid.cpp:150-288).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

namespace o3dmi {

// floor(p / grid_size) of one point and the two trilinear weights per axis.
struct Cell {
    int k[3];
    float fl[3];
    float r[3][2];  // r[axis][0] = 1 - residual, r[axis][1] = residual
};

// False for a non-finite coordinate and for a cell whose far corner leaves the
// hash's key range (upstream's float -> int32 cast is undefined there).
__device__ __forceinline__ bool Quantize(const float* __restrict__ p,
                                         float grid_size, Cell& c) {
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = p[a] / grid_size;
        const float fl = floorf(q);
        // the comparisons are false for NaN
        ok = ok && fl >= -(float)kKeyBias && fl <= (float)(kKeyBias - 2);
        const float res = q - fl;
        c.fl[a] = fl;
        c.k[a] = ok ? (int)fl : 0;
        c.r[a][0] = 1.f - res;
        c.r[a][1] = res;
    }
    return ok;
}

// Buffer indices of the eight corners (nb = x_sel << 2 | y_sel << 1 | z_sel);
// false when one is missing.
__device__ __forceinline__ bool FindCorners(const HashView& hv, const Cell& c,
                                            int (&idx)[8]) {
    bool all = true;
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) {
        idx[nb] = hv.Find(c.k[0] + ((nb >> 2) & 1), c.k[1] + ((nb >> 1) & 1),
                          c.k[2] + (nb & 1));
        all = all && idx[nb] >= 0;
    }
    return all;
}

__device__ __forceinline__ float VertexRatio(const Cell& c, int nb) {
    return (c.r[0][(nb >> 2) & 1] * c.r[1][(nb >> 1) & 1]) * c.r[2][nb & 1];
}

__device__ __forceinline__ float NormalRatio(const Cell& c, int nb,
                                             const float* __restrict__ nm) {
    const int xs = (nb >> 2) & 1, ys = (nb >> 1) & 1, zs = nb & 1;
    const float sx = xs * 2.0f - 1.0f, sy = ys * 2.0f - 1.0f,
                sz = zs * 2.0f - 1.0f;
    const float a = ((sx * nm[0]) * c.r[1][ys]) * c.r[2][zs];
    const float b = ((sy * nm[1]) * c.r[0][xs]) * c.r[2][zs];
    const float d = ((sz * nm[2]) * c.r[0][xs]) * c.r[1][ys];
    return (a + b) + d;
}

// sum_k ratio[k] * rows[idx[k]] in k order.
__device__ __forceinline__ void Interpolate(const float* __restrict__ rows,
                                            const int (&idx)[8],
                                            const float (&ratio)[8],
                                            float (&out)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = ratio[0] * rows[3 * (int64_t)idx[0] + a];
#pragma unroll
    for (int k = 1; k < 8; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a)
            out[a] = out[a] + ratio[k] * rows[3 * (int64_t)idx[k] + a];
}

}  // namespace o3dmi
