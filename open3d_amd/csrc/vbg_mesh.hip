// Marching cubes over the TSDF voxel blocks on MI355X: replaces
// ExtractTriangleMeshCUDA<tsdf_t, weight_t, color_t>
// (cpp/open3d/t/geometry/kernel/VoxelBlockGridImpl.h:1383-1783, passes 0-3)
// together with the host-side BufferRadiusNeighbors table and inverse index
// map (t/geometry/VoxelBlockGrid.cpp:436-471). Tables: mc_tables.h, generated
// by tools/gen_mc_tables.py (same edge masks, vertices, polygons and
// orientation as the reference's; the diagonal inside a patch of 4 or more
// vertices may differ).
//
// Differences in structure (same per-vertex arithmetic as pass 2):
//  * no {n_blocks, R^3, 4} mesh_structure (40 GB at 623 k blocks): one
//    workgroup owns one active block, looks its 27 neighbours up in the
//    spatial hash into LDS and loads a one-voxel halo of (weight > threshold,
//    tsdf < 0) bits, (R+2)^3 bytes of LDS. A cube is valid when its 8 corners
//    are; a voxel's edge along axis a has a vertex when its ends differ in
//    sign and one of the (up to 4) valid cubes around it holds it -- the
//    gather form of pass 0, no cross-block writes;
//  * count (vertices and triangles per block) -> device scan -> write: the
//    vertex pass writes each vertex at offset(block) + rank(voxel, axis) and
//    each voxel's first vertex index (4 B per voxel of the active blocks, the
//    only scratch proportional to the grid); the triangle pass reads those
//    for its own voxels and the +x / +y / +z neighbours' first layers. Output
//    order: vertices by (active block, voxel, axis), triangles by (active
//    block, voxel, table order) -- identical on every run, where the
//    reference's is its atomic counters';
//  * a capacity check on the device before any write: too small a vertex or
//    triangle capacity writes nothing (the reference writes past its
//    tensors);
//  * 64-bit linear voxel indices.
// The per-voxel arithmetic (neighbour lookup, normals, edge vertices) is
// vbg_surface.h's, shared with vbg_extract.hip.

#include "mc_tables.h"
#include "scan.h"
#include "vbg_surface.h"

namespace o3dmi {
namespace {

constexpr int kMeshBlock = 256;
constexpr int kMaxMeshRes = 32;  // (R+2)^3 bytes of LDS: 39 KB at R = 32

// Halo cell bits.
constexpr unsigned char kOk = 1;    // voxel exists and weight > threshold
constexpr unsigned char kNeg = 2;   // tsdf < 0
constexpr unsigned char kCube = 4;  // the cube with its origin here is valid

// Bit 31 of a voxel's first-vertex word: the voxel has a vertex on axis 0.
constexpr unsigned kHas0 = 0x80000000u;

struct MeshArgs {
    const int32_t* indices;  // [n_blocks] active buffer indices, ascending
    int n_blocks;
    const float* tsdf;
    const void* weight;
    const void* color;
    int resolution;
    float voxel_size;
    float weight_threshold;
    const long long* totals;  // [2] vertices, triangles (after the scan)
    long long vertex_capacity;
    long long triangle_capacity;
};

// Halo index of voxel (x, y, z), each in [-1, R].
__device__ __forceinline__ int H(int x, int y, int z, int s) {
    return ((z + 1) * s + (y + 1)) * s + (x + 1);
}

// LoadNeighbours (key into xyz_b, 27 neighbours into nb), then the (R+2)^3
// halo cells into `cell`: kOk / kNeg per voxel, then kCube per cube origin in
// [-1, R-1]^3. Ends with a barrier.
template <typename weight_t, int RT>
__device__ void LoadBlock(const HashView& hv, const MeshArgs& a, Res<RT> rs,
                          int block_idx, int* nb, unsigned char* cell,
                          int* xyz_b) {
    const int res = rs.r;
    const int s = res + 2;
    const int s3 = s * s * s;
    LoadNeighbours(hv, block_idx, nb, xyz_b);
    const weight_t* __restrict__ weight = (const weight_t*)a.weight;
    const float thr = a.weight_threshold;
    for (int h = threadIdx.x; h < s3; h += kMeshBlock) {
        const int x = h % s - 1, y = (h / s) % s - 1, z = h / (s * s) - 1;
        const long long li = LinearIdx(x, y, z, rs, nb);
        unsigned char c = 0;
        if (li >= 0) {
            // pass 0 (:1478-1486): weight_i <= weight_threshold -> no cube
            if (!((float)weight[li] <= thr)) c |= kOk;
            if (a.tsdf[li] < 0) c |= kNeg;
        }
        cell[h] = c;
    }
    __syncthreads();
    const int c1 = res + 1;
    for (int h = threadIdx.x; h < c1 * c1 * c1; h += kMeshBlock) {
        const int x = h % c1 - 1, y = (h / c1) % c1 - 1, z = h / (c1 * c1) - 1;
        const int o = H(x, y, z, s);
        const int sy = s, sz = s * s;
        const unsigned char all = cell[o] & cell[o + 1] & cell[o + sy] &
                                  cell[o + sy + 1] & cell[o + sz] &
                                  cell[o + sz + 1] & cell[o + sz + sy] &
                                  cell[o + sz + sy + 1];
        if (all & kOk) cell[o] |= kCube;
    }
    __syncthreads();
}

// Axes of voxel (x, y, z) in [0, R)^3 whose edge holds a vertex (bit a).
__device__ __forceinline__ int VertexFlags(const unsigned char* cell, int x,
                                           int y, int z, int s) {
    const int o = H(x, y, z, s);
    const int step[3] = {1, s, s * s};
    const int neg = cell[o] & kNeg;
    int flags = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if ((cell[o + step[ax]] & kNeg) == neg) continue;
        const int b = step[(ax + 1) % 3], c = step[(ax + 2) % 3];
        if ((cell[o] | cell[o - b] | cell[o - c] | cell[o - b - c]) & kCube)
            flags |= 1 << ax;
    }
    return flags;
}

// Marching-cubes case of the cube at (x, y, z) in [0, R)^3; -1 if invalid.
__device__ __forceinline__ int CubeCase(const unsigned char* cell, int x,
                                        int y, int z, int s) {
    const int o = H(x, y, z, s);
    if (!(cell[o] & kCube)) return -1;
    int c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = o + mc::kCorner[i][0] + mc::kCorner[i][1] * s +
                      mc::kCorner[i][2] * s * s;
        if (cell[k] & kNeg) c |= 1 << i;
    }
    return c;
}

// Pass 1: vertices and triangles per active block.
template <typename weight_t, int RT>
__global__ void __launch_bounds__(kMeshBlock)
MeshCountKernel(HashView hv, MeshArgs a, int* __restrict__ vcount,
                int* __restrict__ tcount) {
    extern __shared__ unsigned char cell[];
    __shared__ int nb[27];
    __shared__ int xyz_b[3];
    __shared__ int wave_sums[kMeshBlock / 64];
    const Res<RT> rs(a.resolution);
    const int res = rs.r, s = res + 2, res3 = res * res * res;
    LoadBlock<weight_t>(hv, a, rs, a.indices[blockIdx.x], nb, cell, xyz_b);
    int vt = 0, tt = 0;
#pragma unroll 1
    for (int v0 = 0; v0 < res3; v0 += kMeshBlock) {
        const int v = v0 + threadIdx.x;
        int nv = 0, nt = 0;
        if (v < res3) {
            int x, y, z;
            rs.Voxel(v, x, y, z);
            nv = __popc(VertexFlags(cell, x, y, z, s));
            const int c = CubeCase(cell, x, y, z, s);
            nt = c < 0 ? 0 : mc::kTriCount[c];
        }
        int sv, st;
        (void)BlockExclusiveScan<kMeshBlock>(nv, wave_sums, sv);
        (void)BlockExclusiveScan<kMeshBlock>(nt, wave_sums, st);
        vt += sv;
        tt += st;
    }
    if (threadIdx.x == 0) {
        vcount[blockIdx.x] = vt;
        tcount[blockIdx.x] = tt;
    }
}

__device__ __forceinline__ bool OverCapacity(const MeshArgs& a) {
    const long long nv = a.totals[0], nt = a.totals[1];
    return nv > a.vertex_capacity || nt > a.triangle_capacity ||
           nv > 0x7fffffffll;
}

// Pass 2 (:1567-1678): vertices, normals, colours; each voxel's first vertex
// index (| kHas0) into vfirst[position * R^3 + voxel], and the total into
// vfirst[n_blocks * R^3].
template <typename weight_t, typename color_t, int RT>
__global__ void __launch_bounds__(kMeshBlock)
MeshVertexKernel(HashView hv, MeshArgs a, const long long* __restrict__ voff,
                 unsigned* __restrict__ vfirst, float* __restrict__ vertices,
                 float* __restrict__ normals, float* __restrict__ colors) {
    extern __shared__ unsigned char cell[];
    __shared__ int nb[27];
    __shared__ int xyz_b[3];
    __shared__ int wave_sums[kMeshBlock / 64];
    if (OverCapacity(a)) return;
    const Res<RT> rs(a.resolution);
    const int res = rs.r, s = res + 2, res3 = res * res * res;
    const int block_idx = a.indices[blockIdx.x];
    LoadBlock<weight_t>(hv, a, rs, block_idx, nb, cell, xyz_b);
    const float* __restrict__ tsdf = a.tsdf;
    const color_t* __restrict__ color = (const color_t*)a.color;
    long long base = voff[blockIdx.x];
    unsigned* __restrict__ vf = vfirst + (long long)blockIdx.x * res3;
    for (int v0 = 0; v0 < res3; v0 += kMeshBlock) {
        const int voxel_idx = v0 + threadIdx.x;
        int flags = 0, xv = 0, yv = 0, zv = 0;
        if (voxel_idx < res3) {
            rs.Voxel(voxel_idx, xv, yv, zv);
            flags = VertexFlags(cell, xv, yv, zv, s);
        }
        int chunk_total;
        const int rank = BlockExclusiveScan<kMeshBlock>(
                __popc(flags), wave_sums, chunk_total);
        long long idx = base + rank;
        if (voxel_idx < res3)
            vf[voxel_idx] = (unsigned)idx | ((flags & 1) ? kHas0 : 0u);
        if (flags) {
            const long long linear_idx = (long long)block_idx * res3 + voxel_idx;
            const float tsdf_o = tsdf[linear_idx];
            float no[3] = {0, 0, 0}, ne[3] = {0, 0, 0};
            GetNormal(tsdf, xv, yv, zv, rs, nb, no);
            for (int e = 0; e < 3; ++e) {
                if (!(flags & (1 << e))) continue;
                EdgeVertex(tsdf, color, rs, nb, xyz_b, xv, yv, zv, e,
                           linear_idx, tsdf_o, no, ne, a.voxel_size, true, idx,
                           vertices, normals, colors);
                ++idx;
            }
        }
        base += chunk_total;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        vfirst[(long long)gridDim.x * res3] = (unsigned)base;
}

// Position of buffer index b in the ascending active list; -1 if absent.
__device__ __forceinline__ int ActivePosition(const int32_t* indices, int n,
                                              int b) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (indices[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && indices[lo] == b) ? lo : -1;
}

// Pass 3 (:1680-1776): triangles of the valid cubes, in table order; the
// table already holds the output orientation.
template <typename weight_t, int RT>
__global__ void __launch_bounds__(kMeshBlock)
MeshTriangleKernel(HashView hv, MeshArgs a, const long long* __restrict__ toff,
                   const unsigned* __restrict__ vfirst,
                   int32_t* __restrict__ triangles, int* __restrict__ err) {
    extern __shared__ unsigned char cell[];
    __shared__ int nb[27];
    __shared__ int pos[27];
    __shared__ int xyz_b[3];
    __shared__ int wave_sums[kMeshBlock / 64];
    if (OverCapacity(a)) return;
    const Res<RT> rs(a.resolution);
    const int res = rs.r, s = res + 2, res3 = res * res * res;
    LoadBlock<weight_t>(hv, a, rs, a.indices[blockIdx.x], nb, cell, xyz_b);
    if (threadIdx.x < 27)
        pos[threadIdx.x] = nb[threadIdx.x] < 0
                                   ? -1
                                   : ActivePosition(a.indices, a.n_blocks,
                                                    nb[threadIdx.x]);
    __syncthreads();
    long long base = toff[blockIdx.x];
    for (int v0 = 0; v0 < res3; v0 += kMeshBlock) {
        const int v = v0 + threadIdx.x;
        int c = -1, xv = 0, yv = 0, zv = 0;
        if (v < res3) {
            rs.Voxel(v, xv, yv, zv);
            c = CubeCase(cell, xv, yv, zv, s);
        }
        const int nt = c < 0 ? 0 : mc::kTriCount[c];
        int chunk_total;
        const int rank =
                BlockExclusiveScan<kMeshBlock>(nt, wave_sums, chunk_total);
        int32_t* tri = triangles + 3 * (base + rank);
        for (int k = 0; k < 3 * nt; ++k) {
            const int j = mc::kTriTable[c][k];
            const int xo = xv + mc::kEdgeOwner[j][0];
            const int yo = yv + mc::kEdgeOwner[j][1];
            const int zo = zv + mc::kEdgeOwner[j][2];
            const int ax = mc::kEdgeOwner[j][3];
            const int dx = xo >= res, dy = yo >= res, dz = zo >= res;
            const int p = pos[(dx + 1) + (dy + 1) * 3 + (dz + 1) * 9];
            int32_t out = -1;
            if (p >= 0) {
                const long long w = (long long)p * res3 +
                                    ((zo - dz * res) * res + (yo - dy * res)) *
                                            res +
                                    (xo - dx * res);
                const unsigned f = vfirst[w];
                const unsigned first = f & ~kHas0;
                const unsigned cnt = (vfirst[w + 1] & ~kHas0) - first;
                // rank of axis `ax` among the voxel's vertices
                const unsigned r = ax == 0   ? 0u
                                   : ax == 2 ? cnt - 1u
                                   : cnt == 2 ? ((f & kHas0) ? 1u : 0u)
                                              : (cnt == 3 ? 1u : 0u);
                out = (int32_t)(first + r);
            } else {
                atomicOr(err, 1);
            }
            tri[k] = out;
        }
        base += chunk_total;
    }
}

}  // namespace
}  // namespace o3dmi

using namespace o3dmi;

extern "C" int o3dmi_vbg_extract_mesh(
        o3dmi_hash_t* block_hash, const int32_t* indices_dev, int64_t n_blocks,
        const float* tsdf_dev, const void* weight_dev, const void* color_dev,
        int grid_dtype, int resolution, float voxel_size,
        float weight_threshold, float* vertices_dev, float* normals_dev,
        float* colors_dev, int32_t* triangles_dev, int64_t vertex_capacity,
        int64_t* n_vertices_out, int64_t* n_triangles_out,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(block_hash && n_vertices_out && n_triangles_out,
                  "null argument");
    *n_vertices_out = 0;
    *n_triangles_out = 0;
    int st = CheckSurfaceArgs(
            n_blocks, resolution, kMaxMeshRes,
            "ExtractTriangleMesh: block resolution must be in [1, 32]",
            grid_dtype, indices_dev, tsdf_dev, weight_dev);
    if (st || n_blocks == 0) return st;
    const bool write = vertex_capacity > 0;
    if (write)
        O3DMI_REQUIRE(vertices_dev && normals_dev && triangles_dev,
                      "null output");
    hipStream_t s = (hipStream_t)stream;
    const int64_t res3 = (int64_t)resolution * resolution * resolution;
    // scratch: [2] totals, [n] vertex offsets, [n] triangle offsets, scan
    // temporary, [n] + [n] counts, [1] error word, and (writing) the
    // first-vertex words [n * R^3 + 1]
    const size_t scan_bytes = (ScanScratchBytes(n_blocks) + 7) / 8 * 8;
    const size_t n = (size_t)n_blocks;
    const size_t fixed = 8 * (2 + 2 * n) + scan_bytes + 4 * (2 * n + 2);
    const size_t first_bytes = write ? 4 * ((size_t)n * res3 + 1) : 0;
    PoolScratch scratch(s);
    char* mem = nullptr;
    if ((st = scratch.Alloc(&mem, fixed + first_bytes))) return st;
    long long* totals = (long long*)mem;
    long long* voff = totals + 2;
    long long* toff = voff + n;
    void* scan_tmp = (void*)(toff + n);
    int* vcount = (int*)((char*)scan_tmp + scan_bytes);
    int* tcount = vcount + n;
    int* err = tcount + n;
    unsigned* vfirst = (unsigned*)(mem + fixed);

    MeshArgs a;
    a.indices = indices_dev;
    a.n_blocks = (int)n_blocks;
    a.tsdf = tsdf_dev;
    a.weight = weight_dev;
    a.color = color_dev;
    a.resolution = resolution;
    a.voxel_size = voxel_size;
    a.weight_threshold = weight_threshold;
    a.totals = totals;
    a.vertex_capacity = vertex_capacity;
    a.triangle_capacity =
            vertex_capacity > 0 ? 3 * (long long)vertex_capacity : 0;
    const dim3 grid((unsigned)n_blocks), block(kMeshBlock);
    const size_t lds = (size_t)(resolution + 2) * (resolution + 2) *
                       (resolution + 2);
    const HashView hv = block_hash->view;
    const bool f32 = grid_dtype == O3DMI_F32;

    hipError_t e = hipMemsetAsync(err, 0, sizeof(int), s);
    if (e == hipSuccess) {
        WithRes(resolution, [&](auto rt) {
            constexpr int RT = decltype(rt)::value;
            if (f32)
                hipLaunchKernelGGL((MeshCountKernel<float, RT>), grid, block,
                                   lds, s, hv, a, vcount, tcount);
            else
                hipLaunchKernelGGL((MeshCountKernel<uint16_t, RT>), grid,
                                   block, lds, s, hv, a, vcount, tcount);
        });
        st = PrefixSumAsync(vcount, n_blocks, false, (int64_t*)voff,
                            (int64_t*)totals, scan_tmp, s);
        if (!st)
            st = PrefixSumAsync(tcount, n_blocks, false, (int64_t*)toff,
                                (int64_t*)(totals + 1), scan_tmp, s);
    }
    if (e == hipSuccess && !st && write) {
        WithRes(resolution, [&](auto rt) {
            constexpr int RT = decltype(rt)::value;
            if (f32) {
                hipLaunchKernelGGL((MeshVertexKernel<float, float, RT>), grid,
                                   block, lds, s, hv, a, voff, vfirst,
                                   vertices_dev, normals_dev, colors_dev);
                hipLaunchKernelGGL((MeshTriangleKernel<float, RT>), grid,
                                   block, lds, s, hv, a, toff, vfirst,
                                   triangles_dev, err);
            } else {
                hipLaunchKernelGGL((MeshVertexKernel<uint16_t, uint16_t, RT>),
                                   grid, block, lds, s, hv, a, voff, vfirst,
                                   vertices_dev, normals_dev, colors_dev);
                hipLaunchKernelGGL((MeshTriangleKernel<uint16_t, RT>), grid,
                                   block, lds, s, hv, a, toff, vfirst,
                                   triangles_dev, err);
            }
        });
    }
    long long host[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && !st)
        e = hipMemcpyAsync(host, totals, 2 * sizeof(long long),
                           hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && !st)
        e = hipMemcpyAsync(&host[2], err, sizeof(int), hipMemcpyDeviceToHost,
                           s);
    hipError_t e2 = hipStreamSynchronize(s);
    if (st) return st;
    O3DMI_HIP_CHECK(e);
    O3DMI_HIP_CHECK(e2);
    *n_vertices_out = (int64_t)host[0];
    *n_triangles_out = (int64_t)host[1];
    if (host[0] > 0x7fffffffll) {
        SetLastError("ExtractTriangleMesh: more than INT32_MAX vertices");
        return O3DMI_ERR_CAPACITY;
    }
    if (vertex_capacity >= 0 &&
        (host[0] > vertex_capacity || host[1] > 3 * (long long)vertex_capacity)) {
        SetLastError("ExtractTriangleMesh: estimated_vertex_number too small "
                     "for the mesh's vertices or triangles (3 per vertex)");
        return O3DMI_ERR_CAPACITY;
    }
    if ((int)host[2] != 0) {
        SetLastError("ExtractTriangleMesh: a neighbour block is missing from "
                     "the active list (indices must be ascending and hold "
                     "every block of the grid)");
        return O3DMI_ERR_INTERNAL;
    }
    return O3DMI_OK;
}
