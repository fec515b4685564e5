// slac::ControlGrid kernels (control_grid.hip): touch, neighbour map,
// trilinear embedding, deformation and the z-buffered projection. The
// stream-ordered launchers host/control_grid.cpp drives; none of them waits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "common.h"

namespace o3dmi {

constexpr unsigned long long kEmptyPacked = 0xFFFFFFFFFFFFFFFFull;

// A world <-> image pair of one frame: `pose` (inverse extrinsic) unprojects,
// `cam` (extrinsic) projects; both carry the intrinsics.
struct ControlGridFrame {
    Camera pose;
    Camera cam;
    int rows, cols;
    float depth_scale, depth_max;
};

ControlGridFrame MakeControlGridFrame(const double* intrinsic,
                                      const double* extrinsic, int rows,
                                      int cols, float depth_scale,
                                      float depth_max);

// Inserts the eight corner nodes of every point, value = key * grid_size
// (value buffer 0 of `h`, {capacity,3} float32). Runs as a frame-stream group
// does: when the map runs out of buffer indices the first overflow is stamped
// in counters[3] and the rest of the launch is dropped (RecoverOverflow,
// Reserve, replay).
int ControlGridTouchAsync(o3dmi_hash* h, const float* points_dev, int64_t n,
                          float grid_size, hipStream_t s);

// {n,6} buffer indices / masks of the -x +x -y +y -z +z neighbours of the
// listed nodes.
int ControlGridNeighborMapAsync(o3dmi_hash* h, const int32_t* active_dev,
                                int64_t n, int32_t* nb_indices_dev,
                                uint8_t* nb_masks_dev, hipStream_t s);

// out[i] = key_buffer[i] * grid_size for all `capacity` rows.
int ControlGridInitPositionsAsync(o3dmi_hash* h, float grid_size,
                                  float* out_dev, hipStream_t s);

// flags[i] = 1 when all eight corners of point i are nodes of the map.
int ControlGridValidAsync(o3dmi_hash* h, const float* points_dev, int64_t n,
                          float grid_size, int32_t* flags_dev, hipStream_t s);

// Row position[i] of every output for the points with flags[i] != 0. normals /
// colors and their outputs may be null.
int ControlGridParameterizeAsync(
        o3dmi_hash* h, const float* points_dev, const float* normals_dev,
        const float* colors_dev, int64_t n, float grid_size,
        const int32_t* flags_dev, const int64_t* position_dev,
        float* out_points_dev, float* out_normals_dev, float* out_colors_dev,
        int32_t* out_indices_dev, float* out_vertex_ratios_dev,
        float* out_normal_ratios_dev, hipStream_t s);

// Two launches: *bad_dev (zeroed by the caller) is set when an index is
// outside [0, capacity); the second launch then writes nothing.
int ControlGridDeformAsync(o3dmi_hash* h, const int32_t* indices_dev,
                           const float* vertex_ratios_dev,
                           const float* normal_ratios_dev, int64_t n,
                           float* out_points_dev, float* out_normals_dev,
                           int* bad_dev, hipStream_t s);

// packed[pixel] = min over the points that land on it of
// (bits of d << 32 | point index); packed_dev is filled with kEmptyPacked
// first.
int ProjectPackAsync(const float* points_dev, int64_t n,
                     const ControlGridFrame& f,
                     unsigned long long* packed_dev, hipStream_t s);

// depth / colour of every pixel from its packed word: the winner's d, and row
// `index` of colors_dev (float32 x 3, or uint8 x 3 scaled by 1/255 as
// Image::To does). colors_dev / color_out_dev may be null.
int ProjectResolveAsync(const unsigned long long* packed_dev, int rows,
                        int cols, const void* colors_dev, int colors_dtype,
                        float* depth_out_dev, float* color_out_dev,
                        hipStream_t s);

// The fused image deformation: pixel -> world point -> eight finds -> deformed
// point -> projection -> packed[target] = min(bits of d << 32 | source pixel).
int ControlGridDeformImagePackAsync(o3dmi_hash* h, const void* depth_dev,
                                    int depth_dtype,
                                    const ControlGridFrame& f, float grid_size,
                                    unsigned long long* packed_dev,
                                    hipStream_t s);

}  // namespace o3dmi
