// o3dmi_preload: loads the code objects of the translation units listed in
// preload.h.

#include "../common.h"
#include "../preload.h"
#include "o3d_mi355x_host.h"

using namespace o3dmi;

// Extension: everything a first frame would otherwise pay for besides its own
// buffers. HIP loads a translation unit's code object at the first launch of
// one of its kernels -- 1.5-2.8 ms each for the large ones (ICP search,
// VoxelDownSample, the search index): of the 8.7 ms a first tracked frame
// took, most was that (profiles/r6k_first_frame.txt). Loads them now; safe to
// call more than once and from any thread.
extern "C" int o3dmi_preload(void) {
    int bad = 0;
    bad += o3dmi::PreloadBlockHash();
    bad += o3dmi::PreloadTouch();
    bad += o3dmi::PreloadStream();
    bad += o3dmi::PreloadRaycast();
    bad += o3dmi::PreloadPointcloud();
    bad += o3dmi::PreloadNns();
    bad += o3dmi::PreloadIcp();
    bad += o3dmi::PreloadStreamDriver();
    if (bad) {
        SetLastError("o3dmi_preload: a code object could not be loaded");
        return O3DMI_ERR_HIP;
    }
    return O3DMI_OK;
}
