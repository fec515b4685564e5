// Surface point extraction from the TSDF voxel blocks on MI355X (SURVEY.md
// section 8 row f2). Replaces ExtractPointCloudCUDA<tsdf_t, weight_t, color_t>
// (cpp/open3d/t/geometry/kernel/VoxelBlockGridImpl.h:1122-1365, helpers
// DeviceGetLinearIdx / DeviceGetNormal :94-149) together with the host-side
// BufferRadiusNeighbors table (t/geometry/VoxelBlockGrid.cpp:22-51).
//
// Differences in structure (same per-point arithmetic):
//  * no {27, n} neighbour tables in HBM: one workgroup owns one active block
//    and its first 27 lanes look the neighbours up in the spatial hash into
//    LDS;
//  * no global atomic counter: pass 1 counts the zero crossings per block,
//    a scan turns the counts into offsets, pass 2 writes each point at
//    offset(block) + rank(voxel, axis) -- the output order is (active block,
//    voxel, axis), identical on every run (the reference's order is whatever
//    its atomic counter hands out);
//  * 64-bit linear indices (the reference's `int` overflows past 524 287
//    blocks of 16^3).
// HBM bound in principle (one pass over tsdf + weight of the active blocks,
// 6 B / voxel, twice) with scattered neighbour reads at block faces. The
// per-voxel arithmetic is vbg_surface.h's, shared with vbg_mesh.hip; the
// counts become offsets through scan.h's PrefixSumAsync.

#include "scan.h"
#include "vbg_surface.h"

namespace o3dmi {
namespace {

constexpr int kExtractBlock = 256;

struct ExtractArgs {
    const int32_t* indices;  // [n_blocks] active buffer indices
    const float* tsdf;
    const void* weight;
    const void* color;
    int resolution;
    float voxel_size;
    float weight_threshold;
};

template <typename weight_t, typename color_t, bool WRITE, int RT>
__global__ void __launch_bounds__(kExtractBlock)
ExtractKernel(HashView hv, ExtractArgs a, int* __restrict__ block_counts,
              const long long* __restrict__ block_offsets,
              float* __restrict__ points, float* __restrict__ normals,
              float* __restrict__ colors, long long capacity) {
    __shared__ int nb[27];
    __shared__ int wave_sums[kExtractBlock / 64];
    const Res<RT> rs(a.resolution);
    const int res3 = rs.r * rs.r * rs.r;
    const int block_idx = a.indices[blockIdx.x];
    int xyz_b[3];
    LoadNeighbours(hv, block_idx, nb, xyz_b);
    const float* __restrict__ tsdf = a.tsdf;
    const weight_t* __restrict__ weight = (const weight_t*)a.weight;
    const color_t* __restrict__ color = (const color_t*)a.color;
    const float thr = a.weight_threshold;
    long long base = WRITE ? block_offsets[blockIdx.x] : 0;
    int block_total = 0;
#pragma unroll 1
    for (int v0 = 0; v0 < res3; v0 += kExtractBlock) {
        const int voxel_idx = v0 + threadIdx.x;
        int flags = 0;
        int xv = 0, yv = 0, zv = 0;
        long long linear_idx = 0;
        float tsdf_o = 0;
        if (voxel_idx < res3) {
            rs.Voxel(voxel_idx, xv, yv, zv);
            linear_idx = (long long)block_idx * res3 + voxel_idx;
            tsdf_o = tsdf[linear_idx];
            const float weight_o = (float)weight[linear_idx];
            if (!(weight_o <= thr)) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const long long li = LinearIdx(xv + (i == 0), yv + (i == 1),
                                                   zv + (i == 2), rs, nb);
                    if (li < 0) continue;
                    const float tsdf_i = tsdf[li];
                    const float weight_i = (float)weight[li];
                    if (weight_i > thr && tsdf_i * tsdf_o < 0) flags |= 1 << i;
                }
            }
        }
        int chunk_total;
        const int rank = BlockExclusiveScan<kExtractBlock>(
                __popc(flags), wave_sums, chunk_total);
        if (WRITE && flags) {
            float no[3] = {0, 0, 0}, ne[3] = {0, 0, 0};
            GetNormal(tsdf, xv, yv, zv, rs, nb, no);
            long long idx = base + rank;
            for (int i = 0; i < 3; ++i) {
                if (!(flags & (1 << i))) continue;
                EdgeVertex(tsdf, color, rs, nb, xyz_b, xv, yv, zv, i,
                           linear_idx, tsdf_o, no, ne, a.voxel_size,
                           idx < capacity, idx, points, normals, colors);
                ++idx;
            }
        }
        base += chunk_total;
        block_total += chunk_total;
    }
    if (!WRITE && threadIdx.x == 0) block_counts[blockIdx.x] = block_total;
}

}  // namespace
}  // namespace o3dmi

using namespace o3dmi;

extern "C" int o3dmi_vbg_extract_points(
        o3dmi_hash_t* block_hash, const int32_t* indices_dev, int64_t n_blocks,
        const float* tsdf_dev, const void* weight_dev, const void* color_dev,
        int grid_dtype, int resolution, float voxel_size,
        float weight_threshold, float* points_dev, float* normals_dev,
        float* colors_dev, int64_t capacity, int64_t* total_out,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(block_hash && total_out, "null argument");
    *total_out = 0;
    int st = CheckSurfaceArgs(n_blocks, resolution, 64, "bad block resolution",
                              grid_dtype, indices_dev, tsdf_dev, weight_dev);
    if (st || n_blocks == 0) return st;
    const bool write = capacity >= 0;
    if (write && capacity > 0)
        O3DMI_REQUIRE(points_dev && normals_dev, "null output");
    hipStream_t s = (hipStream_t)stream;
    // scratch: [n + 1] offsets (the total last), [n] counts, scan temporary
    PoolScratch scratch(s);
    long long* offsets = nullptr;
    int* counts = nullptr;
    void* scan_tmp = nullptr;
    if ((st = scratch.Alloc(&offsets, sizeof(long long) * (n_blocks + 1))) ||
        (st = scratch.Alloc(&counts, sizeof(int) * n_blocks)) ||
        (st = scratch.Alloc(&scan_tmp, ScanScratchBytes(n_blocks))))
        return st;
    ExtractArgs a;
    a.indices = indices_dev;
    a.tsdf = tsdf_dev;
    a.weight = weight_dev;
    a.color = color_dev;
    a.resolution = resolution;
    a.voxel_size = voxel_size;
    a.weight_threshold = weight_threshold;
    const dim3 grid((unsigned)n_blocks), block(kExtractBlock);
    const HashView hv = block_hash->view;
    const bool f32 = grid_dtype == O3DMI_F32;
    const auto extract = [&](auto rt, auto write_c) {
        constexpr int RT = decltype(rt)::value;
        constexpr bool WR = decltype(write_c)::value;
        if (f32)
            hipLaunchKernelGGL((ExtractKernel<float, float, WR, RT>), grid,
                               block, 0, s, hv, a, counts, offsets, points_dev,
                               normals_dev, colors_dev, (long long)capacity);
        else
            hipLaunchKernelGGL((ExtractKernel<uint16_t, uint16_t, WR, RT>),
                               grid, block, 0, s, hv, a, counts, offsets,
                               points_dev, normals_dev, colors_dev,
                               (long long)capacity);
    };
    WithRes(resolution, [&](auto rt) { extract(rt, std::false_type()); });
    st = PrefixSumAsync(counts, n_blocks, false, (int64_t*)offsets,
                        (int64_t*)(offsets + n_blocks), scan_tmp, s);
    if (!st && write && capacity > 0)
        WithRes(resolution, [&](auto rt) { extract(rt, std::true_type()); });
    long long total = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !st)
        e = hipMemcpyAsync(&total, offsets + n_blocks, sizeof(long long),
                           hipMemcpyDeviceToHost, s);
    hipError_t e2 = hipStreamSynchronize(s);
    if (st) return st;
    O3DMI_HIP_CHECK(e);
    O3DMI_HIP_CHECK(e2);
    *total_out = (int64_t)total;
    return O3DMI_OK;
}
