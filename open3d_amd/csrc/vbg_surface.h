// Surface-extraction core shared by ExtractPointCloud (vbg_extract.hip) and
// ExtractTriangleMesh (vbg_mesh.hip): the reference keeps these in one place
// too (VoxelBlockGridImpl.h:94-149 and the edge-vertex interpolation of both
// extractions). One workgroup owns one active block and reads its 27
// neighbours through an LDS table `nb` of buffer indices (-1 = absent).
// Device helpers, plus the argument checks both seams share.
#pragma once

#include <type_traits>

#include "common.h"

namespace o3dmi {
namespace {

// Block resolution. RT > 0 is a compile-time power of two (8, 16); kResPow2 a
// run-time power of two, kResAny any run-time value. A division by a run-time
// value costs tens of instructions: a run-time power of two uses a mask and a
// shift. Every argument of Mod / Div is non-negative.
constexpr int kResPow2 = 0;
constexpr int kResAny = -1;

template <int RT>
struct Res {
    static_assert(RT == kResAny || RT == kResPow2 ||
                          (RT > 0 && (RT & (RT - 1)) == 0),
                  "compile-time resolutions are powers of two");
    int r, shift;  // shift: kResPow2 only
    __device__ __forceinline__ explicit Res(int res)
        : r(RT > 0 ? RT : res), shift(31 - __clz(res)) {}
    __device__ __forceinline__ int Mod(int x) const {
        return RT > 0 ? x % RT : RT == kResAny ? x % r : (x & (r - 1));
    }
    __device__ __forceinline__ int Div(int x) const {
        return RT > 0 ? x / RT : RT == kResAny ? x / r : (x >> shift);
    }
    // voxel (x, y, z) of linear voxel index v in [0, r^3)
    __device__ __forceinline__ void Voxel(int v, int& x, int& y, int& z) const {
        x = Mod(v);
        y = Mod(Div(v));
        z = Div(Div(v));
    }
};

// Calls f(std::integral_constant<int, RT>) with the form that fits `res`.
template <typename F>
void WithRes(int res, F&& f) {
    if (res == 16) f(std::integral_constant<int, 16>());
    else if (res == 8) f(std::integral_constant<int, 8>());
    else if ((res & (res - 1)) == 0) f(std::integral_constant<int, kResPow2>());
    else f(std::integral_constant<int, kResAny>());
}

__device__ __forceinline__ int Sgn(int x) { return (x > 0) - (x < 0); }

// DeviceGetLinearIdx, VoxelBlockGridImpl.h:94-121. xo, yo, zo in [-R, 2R],
// and 2R only at R = 1: EdgeVertex's GetNormal at the edge's far end reads
// offset R + 1. Offset 2R maps to voxel 0 of the +1 neighbour, not of the +2
// one, as in the reference; the oracles keep that.
template <int RT>
__device__ __forceinline__ long long LinearIdx(int xo, int yo, int zo,
                                               Res<RT> rs, const int* nb) {
    const int res = rs.r;
    const int xn = rs.Mod(xo + res);
    const int yn = rs.Mod(yo + res);
    const int zn = rs.Mod(zo + res);
    const int nb_idx = (Sgn(xo - xn) + 1) + (Sgn(yo - yn) + 1) * 3 +
                       (Sgn(zo - zn) + 1) * 9;
    const int b = nb[nb_idx];
    if (b < 0) return -1;
    return ((((long long)b * res) + zn) * res + yn) * res + xn;
}

// DeviceGetNormal, :123-149: components are only overwritten when both
// neighbours exist.
template <int RT>
__device__ __forceinline__ void GetNormal(const float* __restrict__ tsdf,
                                          int xo, int yo, int zo, Res<RT> rs,
                                          const int* nb, float* n) {
    const long long vxp = LinearIdx(xo + 1, yo, zo, rs, nb);
    const long long vxn = LinearIdx(xo - 1, yo, zo, rs, nb);
    const long long vyp = LinearIdx(xo, yo + 1, zo, rs, nb);
    const long long vyn = LinearIdx(xo, yo - 1, zo, rs, nb);
    const long long vzp = LinearIdx(xo, yo, zo + 1, rs, nb);
    const long long vzn = LinearIdx(xo, yo, zo - 1, rs, nb);
    if (vxp >= 0 && vxn >= 0) n[0] = tsdf[vxp] - tsdf[vxn];
    if (vyp >= 0 && vyn >= 0) n[1] = tsdf[vyp] - tsdf[vyn];
    if (vzp >= 0 && vzn >= 0) n[2] = tsdf[vzp] - tsdf[vzn];
}

// Exclusive prefix of v over a workgroup of kThreads; total = sum over the
// workgroup. wave_sums: kThreads / 64 ints of LDS.
template <int kThreads>
__device__ __forceinline__ int BlockExclusiveScan(int v, int* wave_sums,
                                                  int& total) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) wave_sums[wave] = x;
    __syncthreads();
    int wave_off = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) {
        const int s = wave_sums[k];
        if (k < wave) wave_off += s;
        total += s;
    }
    __syncthreads();
    return wave_off + x - v;
}

// The key of block `block_idx` into xyz_b, and its 27 neighbours' buffer
// indices (the host-side BufferRadiusNeighbors table, VoxelBlockGrid.cpp:
// 22-51) into nb, 13 being the block itself. Ends with a barrier.
__device__ __forceinline__ void LoadNeighbours(const HashView& hv,
                                               int block_idx, int* nb,
                                               int* xyz_b) {
    const int* key = hv.key_buffer + 3 * (long long)block_idx;
    const int xb = key[0], yb = key[1], zb = key[2];
    xyz_b[0] = xb, xyz_b[1] = yb, xyz_b[2] = zb;
    if (threadIdx.x < 27) {
        const int t = threadIdx.x;
        const int dz = t / 9, dy = (t % 9) / 3, dx = t % 3;
        nb[t] = (t == 13) ? block_idx
                          : hv.Find(xb + dx - 1, yb + dy - 1, zb + dz - 1);
    }
    __syncthreads();
}

// The vertex on axis e of voxel (xv, yv, zv) of block xyz_b, whose linear
// index is linear_idx and tsdf tsdf_o (ExtractPointCloud :1305-1364,
// ExtractTriangleMesh pass 2 :1659-1710): position, normal and, when both
// colour pointers are set, colour, into row idx -- written only if `write`.
// `no` is the voxel's GetNormal; `ne` carries over between the axes of a
// voxel as in the reference (it is never reset), so it is updated either way.
template <typename color_t, int RT>
__device__ __forceinline__ void EdgeVertex(
        const float* __restrict__ tsdf, const color_t* __restrict__ color,
        Res<RT> rs, const int* nb, const int* xyz_b, int xv, int yv, int zv,
        int e, long long linear_idx, float tsdf_o, const float* no, float* ne,
        float voxel_size, bool write, long long idx, float* __restrict__ points,
        float* __restrict__ normals, float* __restrict__ colors) {
    const long long linear_idx_e =
            LinearIdx(xv + (e == 0), yv + (e == 1), zv + (e == 2), rs, nb);
    const float tsdf_e = tsdf[linear_idx_e];
    const float ratio = (0 - tsdf_o) / (tsdf_e - tsdf_o);
    GetNormal(tsdf, xv + (e == 0), yv + (e == 1), zv + (e == 2), rs, nb, ne);
    if (!write) return;
    const int x = xyz_b[0] * rs.r + xv;
    const int y = xyz_b[1] * rs.r + yv;
    const int z = xyz_b[2] * rs.r + zv;
    const float nx = (1 - ratio) * no[0] + ratio * ne[0];
    const float ny = (1 - ratio) * no[1] + ratio * ne[1];
    const float nz = (1 - ratio) * no[2] + ratio * ne[2];
    const float norm =
            (float)((double)sqrtf(nx * nx + ny * ny + nz * nz) + 1e-5);
    float* nn = normals + 3 * idx;
    nn[0] = nx / norm;
    nn[1] = ny / norm;
    nn[2] = nz / norm;
    float* p = points + 3 * idx;
    p[0] = voxel_size * ((float)x + ratio * (float)(int)(e == 0));
    p[1] = voxel_size * ((float)y + ratio * (float)(int)(e == 1));
    p[2] = voxel_size * ((float)z + ratio * (float)(int)(e == 2));
    if (color != nullptr && colors != nullptr) {
        const color_t* co = color + 3 * linear_idx;
        const color_t* ce = color + 3 * linear_idx_e;
        const float r_o = (float)co[0], g_o = (float)co[1], b_o = (float)co[2];
        const float r_e = (float)ce[0], g_e = (float)ce[1], b_e = (float)ce[2];
        float* c = colors + 3 * idx;
        c[0] = ((1 - ratio) * r_o + ratio * r_e) / 255.0f;
        c[1] = ((1 - ratio) * g_o + ratio * g_e) / 255.0f;
        c[2] = ((1 - ratio) * b_o + ratio * b_e) / 255.0f;
    }
}

// The checks both extraction seams make of the grid arguments; resolutions
// up to max_res, with `res_message` past it.
inline int CheckSurfaceArgs(int64_t n_blocks, int resolution, int max_res,
                            const char* res_message, int grid_dtype,
                            const int32_t* indices_dev, const float* tsdf_dev,
                            const void* weight_dev) {
    O3DMI_REQUIRE(n_blocks >= 0 && n_blocks < (1ll << 31),
                  "n_blocks out of range");
    O3DMI_REQUIRE(resolution > 0 && resolution <= max_res, res_message);
    O3DMI_REQUIRE(grid_dtype == O3DMI_F32 || grid_dtype == O3DMI_U16,
                  "Unsupported value data type combination. Expected (float, "
                  "float) or (uint16, uint16)");
    O3DMI_REQUIRE(n_blocks == 0 || (indices_dev && tsdf_dev && weight_dev),
                  "TSDF and/or weight not allocated in blocks, please "
                  "implement customized integration.");
    return O3DMI_OK;
}

}  // namespace
}  // namespace o3dmi
