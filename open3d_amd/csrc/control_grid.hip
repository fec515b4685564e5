// slac::ControlGrid on the block hash (t/pipelines/slac/ControlGrid.cpp):
//
//   Touch                 :46-80    TouchKernel (insert fed from the kernel)
//   GetNeighborGridMap    :114-148  NeighborMapKernel
//   Parameterize          :150-239  ValidKernel -> scan -> ParameterizeKernel
//   Deform (cloud)        :241-288  DeformCheckKernel, DeformKernel
//   Deform (image)        :290-322  DeformImagePackKernel -> ResolveKernel
//   Project               PointCloudCUDA.cu:26-160  ProjectPackKernel -> ResolveKernel
//
// All arithmetic is float32 in the reference's operation order (the library is
// compiled with -ffp-contract=off). A node's row is 12 bytes of key and 12
// bytes of position; a grid of a few thousand nodes stays in L2, so the
// per-point traffic that reaches HBM is the point's own rows.
#include "control_grid.h"

#include "control_grid_device.h"
#include "touch_device.h"

namespace o3dmi {

namespace {

// Project of PointCloudCUDA.cu:53-71: the target pixel and d of one world
// point, false when the point is skipped.
__device__ __forceinline__ bool ProjectPoint(const ControlGridFrame& f,
                                             float x, float y, float z,
                                             int64_t& pixel, float& d) {
    float xc, yc, zc, u, v;
    f.cam.RigidTransform(x, y, z, xc, yc, zc);
    f.cam.Project(xc, yc, zc, u, v);
    u = roundf(u);
    v = roundf(v);
    if (!InBoundary2D(u, v, f.rows, f.cols) || zc <= 0 || zc > f.depth_max)
        return false;
    pixel = (int64_t)v * f.cols + (int64_t)u;
    d = zc * f.depth_scale;
    return true;
}

__device__ __forceinline__ void PackMin(unsigned long long* packed,
                                        int64_t pixel, float d,
                                        int64_t index) {
    const unsigned long long val =
            ((unsigned long long)__float_as_uint(d) << 32) |
            (unsigned long long)(unsigned)index;
    atomicMin(&packed[pixel], val);
}

__global__ void __launch_bounds__(kBlock)
TouchKernel(HashView hv, const float* __restrict__ points, int64_t n,
            float grid_size, float* __restrict__ values) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        Cell c;
        if (!Quantize(points + 3 * i, grid_size, c)) continue;
#pragma unroll
        for (int nb = 0; nb < 8; ++nb) {
            const int d[3] = {(nb >> 2) & 1, (nb >> 1) & 1, nb & 1};
            unsigned slot = 0;
            if (!InsertKey<true>(hv, c.k[0] + d[0], c.k[1] + d[1],
                                 c.k[2] + d[2], slot, 1))
                continue;
            // created here: -1 marks a key that found no buffer index
            const int idx = __hip_atomic_load(&hv.slot_vals[slot],
                                              __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
            if (idx < 0 || idx >= hv.capacity) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                values[3 * (int64_t)idx + a] =
                        (c.fl[a] + (float)d[a]) * grid_size;
        }
    }
}

__global__ void __launch_bounds__(kBlock)
NeighborMapKernel(HashView hv, const int32_t* __restrict__ active, int64_t n,
                  int32_t* __restrict__ nb_indices,
                  uint8_t* __restrict__ nb_masks) {
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < 6 * n;
         w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = w / 6;
        const int dir = (int)(w % 6);
        const int idx = active[i];
        int found = -1;
        if (idx >= 0 && idx < hv.capacity) {
            int k[3] = {hv.key_buffer[3 * idx + 0], hv.key_buffer[3 * idx + 1],
                        hv.key_buffer[3 * idx + 2]};
            k[dir >> 1] += (dir & 1) ? 1 : -1;
            found = hv.Find(k[0], k[1], k[2]);
        }
        nb_indices[w] = found < 0 ? 0 : found;
        nb_masks[w] = found >= 0;
    }
}

__global__ void __launch_bounds__(kBlock)
InitPositionsKernel(const int* __restrict__ key_buffer, int64_t n3,
                    float grid_size, float* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n3;
         i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (float)key_buffer[i] * grid_size;
}

__global__ void __launch_bounds__(kBlock)
ValidKernel(HashView hv, const float* __restrict__ points, int64_t n,
            float grid_size, int32_t* __restrict__ flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        Cell c;
        int idx[8];
        flags[i] = Quantize(points + 3 * i, grid_size, c) &&
                   FindCorners(hv, c, idx);
    }
}

__global__ void __launch_bounds__(kBlock)
ParameterizeKernel(HashView hv, const float* __restrict__ points,
                   const float* __restrict__ normals,
                   const float* __restrict__ colors, int64_t n,
                   float grid_size, const int32_t* __restrict__ flags,
                   const int64_t* __restrict__ position,
                   float* __restrict__ out_points,
                   float* __restrict__ out_normals,
                   float* __restrict__ out_colors,
                   int32_t* __restrict__ out_indices,
                   float* __restrict__ out_vratios,
                   float* __restrict__ out_nratios) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!flags[i]) continue;
        Cell c;
        int idx[8];
        // the map did not change since ValidKernel: both succeed
        if (!Quantize(points + 3 * i, grid_size, c) ||
            !FindCorners(hv, c, idx))
            continue;
        const int64_t o = position[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) out_points[3 * o + a] = points[3 * i + a];
        if (colors && out_colors)
#pragma unroll
            for (int a = 0; a < 3; ++a)
                out_colors[3 * o + a] = colors[3 * i + a];
#pragma unroll
        for (int nb = 0; nb < 8; ++nb) {
            out_indices[8 * o + nb] = idx[nb];
            out_vratios[8 * o + nb] = VertexRatio(c, nb);
        }
        if (normals) {
            const float nm[3] = {normals[3 * i + 0], normals[3 * i + 1],
                                 normals[3 * i + 2]};
            if (out_normals)
#pragma unroll
                for (int a = 0; a < 3; ++a) out_normals[3 * o + a] = nm[a];
            if (out_nratios)
#pragma unroll
                for (int nb = 0; nb < 8; ++nb)
                    out_nratios[8 * o + nb] = NormalRatio(c, nb, nm);
        }
    }
}

__global__ void __launch_bounds__(kBlock)
DeformCheckKernel(const int32_t* __restrict__ indices, int64_t n8,
                  int capacity, int* __restrict__ bad) {
    bool any = false;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int v = indices[i];
        any = any || v < 0 || v >= capacity;
    }
    if (any) atomicOr(bad, 1);
}

__global__ void __launch_bounds__(kBlock)
DeformKernel(const float* __restrict__ curr,
             const int32_t* __restrict__ indices,
             const float* __restrict__ vratios,
             const float* __restrict__ nratios, int64_t n,
             float* __restrict__ out_points, float* __restrict__ out_normals,
             const int* __restrict__ bad) {
    if (*bad) return;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        int idx[8];
        float ratio[8], v[3];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            idx[k] = indices[8 * i + k];
            ratio[k] = vratios[8 * i + k];
        }
        Interpolate(curr, idx, ratio, v);
#pragma unroll
        for (int a = 0; a < 3; ++a) out_points[3 * i + a] = v[a];
        if (nratios && out_normals) {
#pragma unroll
            for (int k = 0; k < 8; ++k) ratio[k] = nratios[8 * i + k];
            Interpolate(curr, idx, ratio, v);
            const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a) out_normals[3 * i + a] = v[a] / len;
        }
    }
}

__global__ void __launch_bounds__(kBlock)
ProjectPackKernel(const float* __restrict__ points, int64_t n,
                  ControlGridFrame f, unsigned long long* __restrict__ packed) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t pixel;
        float d;
        if (ProjectPoint(f, points[3 * i + 0], points[3 * i + 1],
                         points[3 * i + 2], pixel, d))
            PackMin(packed, pixel, d, i);
    }
}

// Image::To(Float32) of a colour channel (t/geometry/kernel/Image.cpp): scale
// 1/255 and the clamp to [FLT_MIN, FLT_MAX] of o3dmi_image_to_float.
__device__ __forceinline__ float ColorToFloat(uint8_t c) {
    float out = static_cast<float>(c) * (float)(1.0 / 255) + 0.0f;
    return out < 1.17549435e-38f ? 1.17549435e-38f : out;
}

template <typename color_t>
__global__ void __launch_bounds__(kBlock)
ResolveKernel(const unsigned long long* __restrict__ packed, int64_t n_pixels,
              const color_t* __restrict__ colors,
              float* __restrict__ depth_out, float* __restrict__ color_out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < n_pixels; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long w = packed[i];
        const bool hit = w != kEmptyPacked;
        depth_out[i] = hit ? __uint_as_float((unsigned)(w >> 32)) : 0.0f;
        if (!colors || !color_out) continue;
        const int64_t src = (int64_t)(unsigned)(w & 0xFFFFFFFFull);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float c = 0.0f;
            if (hit) {
                if constexpr (sizeof(color_t) == 1)
                    c = ColorToFloat((uint8_t)colors[3 * src + a]);
                else
                    c = (float)colors[3 * src + a];
            }
            color_out[3 * i + a] = c;
        }
    }
}

template <typename depth_t>
__global__ void __launch_bounds__(kBlock)
DeformImagePackKernel(HashView hv, const float* __restrict__ curr,
                      const depth_t* __restrict__ depth, ControlGridFrame f,
                      float grid_size,
                      unsigned long long* __restrict__ packed) {
    const int64_t n = (int64_t)f.rows * f.cols;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        // UnprojectKernel's pixel (vbg_touch.hip), stride 1
        const float dd = (float)depth[i] / f.depth_scale;
        if (!(dd > 0 && dd < f.depth_max)) continue;
        const int64_t y = i / f.cols, x = i % f.cols;
        float xc, yc, zc, p[3];
        f.pose.Unproject((float)x, (float)y, dd, xc, yc, zc);
        f.pose.RigidTransform(xc, yc, zc, p[0], p[1], p[2]);
        Cell c;
        int idx[8];
        if (!Quantize(p, grid_size, c) || !FindCorners(hv, c, idx)) continue;
        float ratio[8], v[3];
#pragma unroll
        for (int nb = 0; nb < 8; ++nb) ratio[nb] = VertexRatio(c, nb);
        Interpolate(curr, idx, ratio, v);
        int64_t pixel;
        float d;
        if (ProjectPoint(f, v[0], v[1], v[2], pixel, d))
            PackMin(packed, pixel, d, i);
    }
}

}  // namespace

ControlGridFrame MakeControlGridFrame(const double* intrinsic,
                                      const double* extrinsic, int rows,
                                      int cols, float depth_scale,
                                      float depth_max) {
    ControlGridFrame f;
    double pose[16];
    InverseTransformation(extrinsic, pose);
    f.pose = Camera::Make(intrinsic, pose, 1.0f);
    f.cam = Camera::Make(intrinsic, extrinsic, 1.0f);
    f.rows = rows;
    f.cols = cols;
    f.depth_scale = depth_scale;
    f.depth_max = depth_max;
    return f;
}

int ControlGridTouchAsync(o3dmi_hash* h, const float* points_dev, int64_t n,
                          float grid_size, hipStream_t s) {
    if (n == 0) return O3DMI_OK;
    hipLaunchKernelGGL(TouchKernel, dim3(GridFor(n, kBlock)), dim3(kBlock), 0,
                       s, h->view, points_dev, n, grid_size,
                       (float*)h->value_buffers[0]);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ControlGridNeighborMapAsync(o3dmi_hash* h, const int32_t* active_dev,
                                int64_t n, int32_t* nb_indices_dev,
                                uint8_t* nb_masks_dev, hipStream_t s) {
    if (n == 0) return O3DMI_OK;
    hipLaunchKernelGGL(NeighborMapKernel, dim3(GridFor(6 * n, kBlock)),
                       dim3(kBlock), 0, s, h->view, active_dev, n,
                       nb_indices_dev, nb_masks_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ControlGridInitPositionsAsync(o3dmi_hash* h, float grid_size,
                                  float* out_dev, hipStream_t s) {
    const int64_t n3 = 3 * h->capacity;
    if (n3 == 0) return O3DMI_OK;
    hipLaunchKernelGGL(InitPositionsKernel, dim3(GridFor(n3, kBlock)),
                       dim3(kBlock), 0, s, h->view.key_buffer, n3, grid_size,
                       out_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ControlGridValidAsync(o3dmi_hash* h, const float* points_dev, int64_t n,
                          float grid_size, int32_t* flags_dev, hipStream_t s) {
    if (n == 0) return O3DMI_OK;
    hipLaunchKernelGGL(ValidKernel, dim3(GridFor(n, kBlock)), dim3(kBlock), 0,
                       s, h->view, points_dev, n, grid_size, flags_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ControlGridParameterizeAsync(
        o3dmi_hash* h, const float* points_dev, const float* normals_dev,
        const float* colors_dev, int64_t n, float grid_size,
        const int32_t* flags_dev, const int64_t* position_dev,
        float* out_points_dev, float* out_normals_dev, float* out_colors_dev,
        int32_t* out_indices_dev, float* out_vertex_ratios_dev,
        float* out_normal_ratios_dev, hipStream_t s) {
    if (n == 0) return O3DMI_OK;
    hipLaunchKernelGGL(ParameterizeKernel, dim3(GridFor(n, kBlock)),
                       dim3(kBlock), 0, s, h->view, points_dev, normals_dev,
                       colors_dev, n, grid_size, flags_dev, position_dev,
                       out_points_dev, out_normals_dev, out_colors_dev,
                       out_indices_dev, out_vertex_ratios_dev,
                       out_normal_ratios_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ControlGridDeformAsync(o3dmi_hash* h, const int32_t* indices_dev,
                           const float* vertex_ratios_dev,
                           const float* normal_ratios_dev, int64_t n,
                           float* out_points_dev, float* out_normals_dev,
                           int* bad_dev, hipStream_t s) {
    if (n == 0) return O3DMI_OK;
    hipLaunchKernelGGL(DeformCheckKernel, dim3(GridFor(8 * n, kBlock)),
                       dim3(kBlock), 0, s, indices_dev, 8 * n,
                       (int)h->capacity, bad_dev);
    hipLaunchKernelGGL(DeformKernel, dim3(GridFor(n, kBlock)), dim3(kBlock), 0,
                       s, (const float*)h->value_buffers[0], indices_dev,
                       vertex_ratios_dev, normal_ratios_dev, n, out_points_dev,
                       out_normals_dev, bad_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ProjectPackAsync(const float* points_dev, int64_t n,
                     const ControlGridFrame& f,
                     unsigned long long* packed_dev, hipStream_t s) {
    O3DMI_HIP_CHECK(hipMemsetAsync(
            packed_dev, 0xFF,
            sizeof(unsigned long long) * (size_t)f.rows * (size_t)f.cols, s));
    if (n == 0) return O3DMI_OK;
    hipLaunchKernelGGL(ProjectPackKernel, dim3(GridFor(n, kBlock)),
                       dim3(kBlock), 0, s, points_dev, n, f, packed_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ProjectResolveAsync(const unsigned long long* packed_dev, int rows,
                        int cols, const void* colors_dev, int colors_dtype,
                        float* depth_out_dev, float* color_out_dev,
                        hipStream_t s) {
    const int64_t n = (int64_t)rows * cols;
    dim3 grid(GridFor(n, kBlock)), block(kBlock);
    if (colors_dev && colors_dtype == O3DMI_U8)
        hipLaunchKernelGGL(ResolveKernel<uint8_t>, grid, block, 0, s,
                           packed_dev, n, (const uint8_t*)colors_dev,
                           depth_out_dev, color_out_dev);
    else
        hipLaunchKernelGGL(ResolveKernel<float>, grid, block, 0, s, packed_dev,
                           n, (const float*)colors_dev, depth_out_dev,
                           color_out_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ControlGridDeformImagePackAsync(o3dmi_hash* h, const void* depth_dev,
                                    int depth_dtype,
                                    const ControlGridFrame& f, float grid_size,
                                    unsigned long long* packed_dev,
                                    hipStream_t s) {
    const int64_t n = (int64_t)f.rows * f.cols;
    O3DMI_HIP_CHECK(hipMemsetAsync(packed_dev, 0xFF,
                                   sizeof(unsigned long long) * (size_t)n, s));
    dim3 grid(GridFor(n, kBlock)), block(kBlock);
    const float* curr = (const float*)h->value_buffers[0];
    if (depth_dtype == O3DMI_U16)
        hipLaunchKernelGGL(DeformImagePackKernel<uint16_t>, grid, block, 0, s,
                           h->view, curr, (const uint16_t*)depth_dev, f,
                           grid_size, packed_dev);
    else
        hipLaunchKernelGGL(DeformImagePackKernel<float>, grid, block, 0, s,
                           h->view, curr, (const float*)depth_dev, f,
                           grid_size, packed_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace o3dmi
