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

#include "common.h"
#include "mc_tables.h"
#include "scan.h"

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

__device__ __forceinline__ int Sgn(int x) { return (x > 0) - (x < 0); }

// Block resolution: RT > 0 is a compile-time value (8, 16), 0 the run-time
// one; divisions by a run-time value cost tens of instructions each.
template <int RT>
struct Res {
    int r;
    __device__ __forceinline__ int R() const { return RT > 0 ? RT : r; }
};

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

// DeviceGetLinearIdx, VoxelBlockGridImpl.h:94-121; nb = LDS table of the 27
// neighbour buffer indices (-1 = absent). xo, yo, zo in [-R, 2R).
template <int RT>
__device__ __forceinline__ long long LinearIdx(int xo, int yo, int zo,
                                               Res<RT> rs, const int* nb) {
    const int res = rs.R();
    const int xn = (xo + res) % res;
    const int yn = (yo + res) % res;
    const int zn = (zo + res) % res;
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

// Exclusive prefix of v over the workgroup; total = sum over the workgroup.
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
    for (int k = 0; k < kMeshBlock / 64; ++k) {
        const int s = wave_sums[k];
        if (k < wave) wave_off += s;
        total += s;
    }
    __syncthreads();
    return wave_off + x - v;
}

// Halo index of voxel (x, y, z), each in [-1, R].
__device__ __forceinline__ int H(int x, int y, int z, int s) {
    return ((z + 1) * s + (y + 1)) * s + (x + 1);
}

// The block's 27 neighbour buffer indices into nb, then the (R+2)^3 halo
// cells into `cell`: kOk / kNeg per voxel, then kCube per cube origin in
// [-1, R-1]^3. Ends with a barrier.
template <typename weight_t, int RT>
__device__ void LoadBlock(const HashView& hv, const MeshArgs& a, Res<RT> rs,
                          int block_idx, int* nb, unsigned char* cell,
                          int* xyz_b) {
    const int res = rs.R();
    const int s = res + 2;
    const int s3 = s * s * s;
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
    Res<RT> rs;
    rs.r = a.resolution;
    const int res = rs.R(), s = res + 2, res3 = res * res * res;
    LoadBlock<weight_t>(hv, a, rs, a.indices[blockIdx.x], nb, cell, xyz_b);
    int vt = 0, tt = 0;
#pragma unroll 1
    for (int v0 = 0; v0 < res3; v0 += kMeshBlock) {
        const int v = v0 + threadIdx.x;
        int nv = 0, nt = 0;
        if (v < res3) {
            const int x = v % res, y = (v / res) % res, z = v / (res * res);
            nv = __popc(VertexFlags(cell, x, y, z, s));
            const int c = CubeCase(cell, x, y, z, s);
            nt = c < 0 ? 0 : mc::kTriCount[c];
        }
        int sv, st;
        (void)BlockExclusiveScan(nv, wave_sums, sv);
        (void)BlockExclusiveScan(nt, wave_sums, st);
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
    Res<RT> rs;
    rs.r = a.resolution;
    const int res = rs.R(), s = res + 2, res3 = res * res * res;
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
            xv = voxel_idx % res;
            yv = (voxel_idx / res) % res;
            zv = voxel_idx / (res * res);
            flags = VertexFlags(cell, xv, yv, zv, s);
        }
        int chunk_total;
        const int rank = BlockExclusiveScan(__popc(flags), wave_sums,
                                            chunk_total);
        long long idx = base + rank;
        if (voxel_idx < res3)
            vf[voxel_idx] = (unsigned)idx | ((flags & 1) ? kHas0 : 0u);
        if (flags) {
            const long long linear_idx = (long long)block_idx * res3 + voxel_idx;
            const float tsdf_o = tsdf[linear_idx];
            float no[3] = {0, 0, 0}, ne[3] = {0, 0, 0};
            GetNormal(tsdf, xv, yv, zv, rs, nb, no);
            const int x = xyz_b[0] * res + xv;
            const int y = xyz_b[1] * res + yv;
            const int z = xyz_b[2] * res + zv;
            // `ne` carries over between the axes of a voxel, as in the
            // reference (it is never reset).
            for (int e = 0; e < 3; ++e) {
                if (!(flags & (1 << e))) continue;
                const long long linear_idx_e = LinearIdx(
                        xv + (e == 0), yv + (e == 1), zv + (e == 2), rs, nb);
                const float tsdf_e = tsdf[linear_idx_e];
                const float ratio = (0 - tsdf_o) / (tsdf_e - tsdf_o);
                float* p = vertices + 3 * idx;
                p[0] = a.voxel_size * ((float)x + ratio * (float)(int)(e == 0));
                p[1] = a.voxel_size * ((float)y + ratio * (float)(int)(e == 1));
                p[2] = a.voxel_size * ((float)z + ratio * (float)(int)(e == 2));
                GetNormal(tsdf, xv + (e == 0), yv + (e == 1), zv + (e == 2),
                          rs, nb, ne);
                const float nx = (1 - ratio) * no[0] + ratio * ne[0];
                const float ny = (1 - ratio) * no[1] + ratio * ne[1];
                const float nz = (1 - ratio) * no[2] + ratio * ne[2];
                const float norm =
                        (float)((double)sqrtf(nx * nx + ny * ny + nz * nz) +
                                1e-5);
                float* nn = normals + 3 * idx;
                nn[0] = nx / norm;
                nn[1] = ny / norm;
                nn[2] = nz / norm;
                if (color != nullptr && colors != nullptr) {
                    const color_t* co = color + 3 * linear_idx;
                    const color_t* ce = color + 3 * linear_idx_e;
                    const float r_o = (float)co[0], g_o = (float)co[1],
                                b_o = (float)co[2];
                    const float r_e = (float)ce[0], g_e = (float)ce[1],
                                b_e = (float)ce[2];
                    float* c = colors + 3 * idx;
                    c[0] = ((1 - ratio) * r_o + ratio * r_e) / 255.0f;
                    c[1] = ((1 - ratio) * g_o + ratio * g_e) / 255.0f;
                    c[2] = ((1 - ratio) * b_o + ratio * b_e) / 255.0f;
                }
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
    Res<RT> rs;
    rs.r = a.resolution;
    const int res = rs.R(), s = res + 2, res3 = res * res * res;
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
            xv = v % res;
            yv = (v / res) % res;
            zv = v / (res * res);
            c = CubeCase(cell, xv, yv, zv, s);
        }
        const int nt = c < 0 ? 0 : mc::kTriCount[c];
        int chunk_total;
        const int rank = BlockExclusiveScan(nt, wave_sums, chunk_total);
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
    O3DMI_REQUIRE(n_blocks >= 0 && n_blocks < (1ll << 31),
                  "n_blocks out of range");
    O3DMI_REQUIRE(resolution > 0 && resolution <= kMaxMeshRes,
                  "ExtractTriangleMesh: block resolution must be in [1, 32]");
    O3DMI_REQUIRE(grid_dtype == O3DMI_F32 || grid_dtype == O3DMI_U16,
                  "Unsupported value data type combination. Expected (float, "
                  "float) or (uint16, uint16)");
    *n_vertices_out = 0;
    *n_triangles_out = 0;
    if (n_blocks == 0) return O3DMI_OK;
    O3DMI_REQUIRE(indices_dev && tsdf_dev && weight_dev,
                  "TSDF and/or weight not allocated in blocks, please implement "
                  "customized integration.");
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
    char* scratch = nullptr;
    int st = PoolAlloc((void**)&scratch, fixed + first_bytes);
    if (st) return st;
    long long* totals = (long long*)scratch;
    long long* voff = totals + 2;
    long long* toff = voff + n;
    void* scan_tmp = (void*)(toff + n);
    int* vcount = (int*)((char*)scan_tmp + scan_bytes);
    int* tcount = vcount + n;
    int* err = tcount + n;
    unsigned* vfirst = (unsigned*)(scratch + fixed);

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

#define O3DMI_MESH_RES(KERNEL_RT, ...)                                         \
    do {                                                                       \
        if (resolution == 16) KERNEL_RT(16, __VA_ARGS__);                      \
        else if (resolution == 8) KERNEL_RT(8, __VA_ARGS__);                   \
        else KERNEL_RT(0, __VA_ARGS__);                                        \
    } while (0)
#define O3DMI_COUNT(RT, WT)                                                    \
    hipLaunchKernelGGL((MeshCountKernel<WT, RT>), grid, block, lds, s, hv, a,  \
                       vcount, tcount)
#define O3DMI_VERTEX(RT, WT)                                                   \
    hipLaunchKernelGGL((MeshVertexKernel<WT, WT, RT>), grid, block, lds, s,    \
                       hv, a, voff, vfirst, vertices_dev, normals_dev,         \
                       colors_dev)
#define O3DMI_TRIANGLE(RT, WT)                                                 \
    hipLaunchKernelGGL((MeshTriangleKernel<WT, RT>), grid, block, lds, s, hv,  \
                       a, toff, vfirst, triangles_dev, err)
    hipError_t e = hipMemsetAsync(err, 0, sizeof(int), s);
    if (e == hipSuccess) {
        if (f32) O3DMI_MESH_RES(O3DMI_COUNT, float);
        else O3DMI_MESH_RES(O3DMI_COUNT, uint16_t);
        st = PrefixSumAsync(vcount, n_blocks, false, (int64_t*)voff,
                            (int64_t*)totals, scan_tmp, s);
        if (!st)
            st = PrefixSumAsync(tcount, n_blocks, false, (int64_t*)toff,
                                (int64_t*)(totals + 1), scan_tmp, s);
    }
    if (e == hipSuccess && !st && write) {
        if (f32) {
            O3DMI_MESH_RES(O3DMI_VERTEX, float);
            O3DMI_MESH_RES(O3DMI_TRIANGLE, float);
        } else {
            O3DMI_MESH_RES(O3DMI_VERTEX, uint16_t);
            O3DMI_MESH_RES(O3DMI_TRIANGLE, uint16_t);
        }
    }
#undef O3DMI_TRIANGLE
#undef O3DMI_VERTEX
#undef O3DMI_COUNT
#undef O3DMI_MESH_RES
    long long host[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && !st)
        e = hipMemcpyAsync(host, totals, 2 * sizeof(long long),
                           hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && !st)
        e = hipMemcpyAsync(&host[2], err, sizeof(int), hipMemcpyDeviceToHost,
                           s);
    hipError_t e2 = hipStreamSynchronize(s);
    PoolFree(scratch);
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
