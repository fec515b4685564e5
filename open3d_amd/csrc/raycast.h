// Private seam between the ray-cast driver (host/vbg_ray_cast.cpp) and its
// kernels' host side (vbg_raycast.hip): the forms of the range estimate and of
// the ray-cast launch that o3dmi_vbg_ray_cast_dev uses with a grid-owned range
// map / block list. The public forms (o3d_mi355x.h) are these with the options
// zeroed.
#pragma once

#include "common.h"

namespace o3dmi {

// What the driver asks of the two launches of one cast beyond their public
// arguments; all zero: nothing.
struct RayCastOptions {
    // The ray cast writes every range cell it reads back to the {lo, hi}
    // stored in the two floats behind the map's last cell (whole-image
    // launches with a down factor of 8 only).
    int reset_range;
    // The ray cast takes its tiles in `order` and writes their durations to
    // `cost` tagged `seq`; the range estimate sorts the `cost` entries tagged
    // `want_seq` into `order` first (n_tiles of them). cost == NULL: tiles in
    // index order, nothing recorded.
    unsigned long long* cost;
    int* order;
    int n_tiles;
    unsigned want_seq, seq;
};

}  // namespace o3dmi

extern "C" {

// o3dmi_vbg_estimate_range_dev where the keys are every `key_stride`-th int
// triple from block_keys_dev; a map the last ray cast left clean skips the
// clearing launch.
int o3dmi_internal_estimate_range(const int32_t* block_keys_dev, int key_stride,
                                  int64_t max_blocks,
                                  const int32_t* n_blocks_dev,
                                  float* range_minmax_map_dev, int map_is_clean,
                                  const double* intrinsic,
                                  const double* extrinsic, int h, int w,
                                  int down_factor, int64_t block_resolution,
                                  float voxel_size, float depth_min,
                                  float depth_max,
                                  const o3dmi::RayCastOptions& options,
                                  o3dmi_stream_t stream);

// o3dmi_vbg_raycast_rows with the options.
int o3dmi_internal_raycast_rows(
        o3dmi_hash_t* block_hash, const float* tsdf_dev, const void* weight_dev,
        const void* color_buf_dev, int grid_dtype, const float* range_map_dev,
        float* out_depth, float* out_vertex, float* out_color,
        float* out_normal, int64_t* out_index, uint8_t* out_mask,
        float* out_ratio, float* out_ratio_dx, float* out_ratio_dy,
        float* out_ratio_dz, const double* intrinsic, const double* extrinsic,
        int h, int w, int row_begin, int row_end, int block_resolution,
        float voxel_size, float depth_scale, float depth_min, float depth_max,
        float weight_threshold, float trunc_voxel_multiplier,
        int range_map_down_factor, const o3dmi::RayCastOptions& options,
        o3dmi_stream_t stream);

}  // extern "C"
