// Kernels of TriangleMesh::SamplePointsUniformly (trianglemesh.h): the prefix
// tree over the triangle areas, its descent per point and upstream's mixing
// (t/geometry/kernel/TriangleMeshCPU.cpp:75-186). A point is a pure function
// of (seed, its index): no state, no atomics besides the error flag.
#include "trianglemesh.h"

#include "mesh_launch.h"

namespace o3dmi {
namespace {

// One thread per group: prefix[i] of the group's values in index order.
template <typename T>
__global__ void GroupPrefixKernel(const T* __restrict__ in, int64_t n,
                                  double* __restrict__ prefix,
                                  int* __restrict__ bad) {
    const int64_t group = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t start = group * kMeshRun;
    if (start >= n) return;
    const int len = (int)(n - start < kMeshRun ? n - start : kMeshRun);
    double sum = 0;
    bool any_bad = false;
    for (int j = 0; j < len; ++j) {
        const double a = (double)in[start + j];
        any_bad |= !(a - a == 0);  // NaN or Inf
        sum = j == 0 ? a : sum + a;
        prefix[start + j] = sum;
    }
    if (any_bad) atomicOr(bad, 1);
}

// next[g] = the last prefix of group g.
__global__ void GroupTotalsKernel(const double* __restrict__ prefix, int64_t n,
                                  double* __restrict__ next, int64_t groups) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    const int64_t last = (g + 1) * kMeshRun < n ? (g + 1) * kMeshRun : n;
    next[g] = prefix[last - 1];
}

inline int64_t GroupsOf(int64_t n) { return (n + kMeshRun - 1) / kMeshRun; }

template <typename T>
__device__ __forceinline__ void Mix3(T* out, const T* a, const T* b,
                                     const T* c, const float wts[3]) {
    out[0] = (wts[0] * a[0] + wts[1] * b[0]) + wts[2] * c[0];
    out[1] = (wts[0] * a[1] + wts[1] * b[1]) + wts[2] * c[1];
    out[2] = (wts[0] * a[2] + wts[1] * b[2]) + wts[2] * c[2];
}

// Vertex colours as upstream's To(Float32), divided by the integer range.
__device__ __forceinline__ void LoadColor(const void* colors, int color_dtype,
                                          int64_t u, float c[3]) {
    for (int k = 0; k < 3; ++k) {
        if (color_dtype == O3DMI_U8)
            c[k] = (float)((const uint8_t*)colors)[3 * u + k] / 255.0f;
        else if (color_dtype == O3DMI_U16)
            c[k] = (float)((const uint16_t*)colors)[3 * u + k] / 65535.0f;
        else
            c[k] = ((const float*)colors)[3 * u + k];
    }
}

template <typename T>
__global__ void SamplePointsKernel(MeshPrefixTree tree,
                                   const T* __restrict__ areas,
                                   MeshSampleIO io, int64_t n, uint64_t seed) {
    const double total =
            tree.prefix[tree.levels - 1][tree.size[tree.levels - 1] - 1];
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n;
         j += (int64_t)gridDim.x * blockDim.x) {
        const MeshSampleDraw d = DrawMeshSample(seed, (uint64_t)j);
        double x = d.u * total;
        int64_t group = 0;
        for (int level = tree.levels - 1; level >= 0; --level) {
            const int64_t base = group * kMeshRun;
            const int64_t left = tree.size[level] - base;
            const int len = (int)(left < kMeshRun ? left : kMeshRun);
            const double* p = tree.prefix[level] + base;
            int lo = 0, hi = len;  // the first i with x < p[i], or len
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (x < p[mid]) hi = mid;
                else lo = mid + 1;
            }
            if (lo == len) {
                // rounding left x at or past the group's total: the last
                // member that can be drawn (the group's total is > 0, so
                // there is one)
                lo = len - 1;
                while (lo > 0) {
                    const int64_t i = base + lo;
                    double own;
                    if (level == 0) {
                        own = (double)areas[i];
                    } else {
                        const int64_t below = tree.size[level - 1];
                        const int64_t last =
                                (i + 1) * kMeshRun < below ? (i + 1) * kMeshRun
                                                           : below;
                        own = tree.prefix[level - 1][last - 1];
                    }
                    if (own > 0) break;
                    --lo;
                }
            }
            if (lo > 0) x -= p[lo - 1];
            group = base + lo;
        }
        const int64_t t = group;
        const float s1 = sqrtf(d.r1);
        const float wts[3] = {1 - s1, s1 * (1 - d.r2), s1 * d.r2};
        const int64_t ia = io.tri[3 * t], ib = io.tri[3 * t + 1],
                      ic = io.tri[3 * t + 2];
        const T* pos = (const T*)io.positions;
        T out[3];
        Mix3(out, pos + 3 * ia, pos + 3 * ib, pos + 3 * ic, wts);
        T* points = (T*)io.points_out;
        points[3 * j] = out[0];
        points[3 * j + 1] = out[1];
        points[3 * j + 2] = out[2];
        if (io.triangles_out) io.triangles_out[j] = (int32_t)t;
        if (io.normals_out) {
            T* normals = (T*)io.normals_out;
            if (io.vertex_normals) {
                const T* vn = (const T*)io.vertex_normals;
                Mix3(out, vn + 3 * ia, vn + 3 * ib, vn + 3 * ic, wts);
            } else {
                const T* tn = (const T*)io.triangle_normals;
                out[0] = tn[3 * t];
                out[1] = tn[3 * t + 1];
                out[2] = tn[3 * t + 2];
            }
            normals[3 * j] = out[0];
            normals[3 * j + 1] = out[1];
            normals[3 * j + 2] = out[2];
        }
        if (io.colors_out) {
            float ca[3], cb[3], cc[3], c[3];
            LoadColor(io.vertex_colors, io.color_dtype, ia, ca);
            LoadColor(io.vertex_colors, io.color_dtype, ib, cb);
            LoadColor(io.vertex_colors, io.color_dtype, ic, cc);
            Mix3(c, ca, cb, cc, wts);
            io.colors_out[3 * j] = c[0];
            io.colors_out[3 * j + 1] = c[1];
            io.colors_out[3 * j + 2] = c[2];
        }
    }
}

}  // namespace

size_t MeshPrefixDoubles(int64_t m) {
    int64_t n = m > 0 ? m : 1;
    size_t total = (size_t)n;
    while (n > kMeshRun) {  // a level's values and its prefixes
        n = GroupsOf(n);
        total += 2 * (size_t)n;
    }
    return total;
}

int MeshPrefixTreeAsync(const void* areas_dev, int64_t m, int dtype,
                        double* prefix_dev, MeshPrefixTree* tree, int* bad_dev,
                        hipStream_t s) {
    O3DMI_REQUIRE(areas_dev && m > 0 && prefix_dev && tree && bad_dev,
                  "null argument");
    const dim3 block(64);
    int64_t n = m;
    double* cursor = prefix_dev;
    const void* values = areas_dev;
    tree->levels = 0;
    for (;;) {
        if (tree->levels == kMeshPrefixLevels) {
            SetLastError("mesh prefix tree: too many levels");
            return O3DMI_ERR_INTERNAL;
        }
        const int64_t groups = GroupsOf(n);
        const dim3 grid((unsigned)GridFor(groups, 64, 1 << 30));
        double* prefix = cursor;
        cursor += n;
        if (tree->levels == 0 && dtype != O3DMI_F64)
            hipLaunchKernelGGL(GroupPrefixKernel<float>, grid, block, 0, s,
                               (const float*)values, n, prefix, bad_dev);
        else
            hipLaunchKernelGGL(GroupPrefixKernel<double>, grid, block, 0, s,
                               (const double*)values, n, prefix, bad_dev);
        tree->size[tree->levels] = n;
        tree->prefix[tree->levels] = prefix;
        ++tree->levels;
        if (groups == 1) break;
        // the next level's values: every group's last prefix
        double* totals = cursor;
        cursor += groups;
        hipLaunchKernelGGL(GroupTotalsKernel, grid, block, 0, s, prefix, n,
                           totals, groups);
        values = totals;
        n = groups;
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int MeshSamplePointsAsync(const MeshPrefixTree& tree, const void* areas_dev,
                          int dtype, const MeshSampleIO& io, int64_t n,
                          uint64_t seed, hipStream_t s) {
    O3DMI_REQUIRE(areas_dev && io.positions && io.tri && io.points_out &&
                          n > 0,
                  "null argument");
    O3DMI_REQUIRE(!io.normals_out || io.vertex_normals || io.triangle_normals,
                  "sample points: normals wanted, none given");
    O3DMI_REQUIRE(!io.colors_out || io.vertex_colors,
                  "sample points: colours wanted, none given");
    if (dtype == O3DMI_F64)
        O3DMI_LAUNCH(SamplePointsKernel<double>, n, tree,
                     (const double*)areas_dev, io, n, seed);
    else
        O3DMI_LAUNCH(SamplePointsKernel<float>, n, tree,
                     (const float*)areas_dev, io, n, seed);
    return O3DMI_OK;
}

}  // namespace o3dmi
