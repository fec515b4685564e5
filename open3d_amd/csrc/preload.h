// o3dmi_preload (host/preload.cpp): one function per translation unit whose
// code object a first frame would otherwise load at its first launch. Each
// asks for the attributes of one of the unit's kernels; 0 on success.
#pragma once

#include <hip/hip_runtime.h>

namespace o3dmi {

inline int LoadCodeObjectOf(const void* kernel) {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, kernel) == hipSuccess ? 0 : 1;
}

int PreloadBlockHash();     // block_hash.hip
int PreloadIcp();           // icp.hip
int PreloadNns();           // nns.hip
int PreloadPointcloud();    // pointcloud.hip
int PreloadRaycast();       // vbg_raycast.hip
int PreloadStream();        // vbg_stream.hip
int PreloadStreamDriver();  // host/vbg_frame_stream.cpp
int PreloadTouch();         // vbg_touch.hip
}  // namespace o3dmi
