// The launch scaffold the TriangleMesh kernel files (trianglemesh*.hip,
// mesh_bvh.hip) share: the grid-stride loop, the grid of a kernel that runs a
// thread per item, the launch of one on the stream `s` in scope, and the grid
// of the kernels that give a wave to every item of a long list.
#pragma once

#include "common.h"

namespace o3dmi {

#define O3DMI_GRID_STRIDE(i, n)                                            \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       \
         i < (n); i += (int64_t)gridDim.x * blockDim.x)

inline dim3 Grid(int64_t n, int block = kBlock) {
    return dim3((unsigned)GridFor(n, block));
}

// The threads of a workgroup O3DMI_LAUNCH starts: kBlock, unless the file
// names a constant of its own before it launches anything.
#ifndef O3DMI_LAUNCH_BLOCK
#define O3DMI_LAUNCH_BLOCK kBlock
#endif

#define O3DMI_LAUNCH(kernel, n, ...)                                       \
    do {                                                                   \
        hipLaunchKernelGGL(kernel, Grid(n, O3DMI_LAUNCH_BLOCK),            \
                           dim3(O3DMI_LAUNCH_BLOCK), 0, s, __VA_ARGS__);   \
        O3DMI_HIP_CHECK(hipGetLastError());                                \
    } while (0)

// A wave per listed item: the grid of the long-list kernels (kBlock threads).
inline dim3 WaveGrid(int64_t n) {
    return dim3((unsigned)GridFor(n, kBlock / 64, kCUs * 8));
}

}  // namespace o3dmi
