// Private seam between slam_model.cpp and the frame-stream driver
// (vbg_frame_stream.cpp).
#pragma once

#include "o3d_mi355x_host.h"

// Copies the block keys the most recent
// o3dmi_vbg_integrate_frame touched (its GetUniqueBlockCoordinates result) to
// out_keys_dev {capacity,3} and their number to out_count_dev, on the stream,
// without a host round trip. Must be issued right behind that call.
extern "C" int o3dmi_vbg_export_last_frame_blocks(
        o3dmi_vbg_t* g, int32_t* out_keys_dev, int64_t out_capacity,
        int32_t* out_count_dev, o3dmi_stream_t stream);
