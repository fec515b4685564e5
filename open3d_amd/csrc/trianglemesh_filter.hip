// Kernels of FilterSharpen / FilterSmoothSimple / FilterSmoothLaplacian /
// FilterSmoothTaubin (trianglemesh_clean.h; legacy geometry/TriangleMesh.cpp:
// 167-440, Smoothing.h:29-65). One pass is one launch for all the attributes
// in scope: a thread walks its vertex's CSR list in order and adds in float64,
// so the result does not depend on the launch geometry; the laplacian's
// weight of a neighbour is computed once and serves every attribute. The walk
// is a dependent gather chain (list entry -> rows), so kFilterWalk entries'
// rows are fetched before the first add. Per pass a vertex reads its list
// (4 B an entry) and 24 B per entry and attribute (and 24 B of position per
// entry for the weights when the positions are not in scope), and writes 24 B
// per attribute: gather-bound, served by L2 / Infinity Cache for a mesh in
// marching-cubes order.
#include "trianglemesh_clean.h"

#include "mesh_launch.h"

namespace o3dmi {
namespace {

template <typename T>
__global__ void WidenKernel(const T* __restrict__ in, int64_t n,
                            double* __restrict__ out) {
    O3DMI_GRID_STRIDE(i, n) out[i] = (double)in[i];
}

template <typename T>
__global__ void NarrowKernel(const double* __restrict__ in, int64_t n,
                             T* __restrict__ out) {
    O3DMI_GRID_STRIDE(i, n) out[i] = (T)in[i];
}

__global__ void LongListsKernel(const int64_t* __restrict__ row_splits,
                                int64_t v, int32_t* __restrict__ long_list) {
    O3DMI_GRID_STRIDE(u, v)
        if (row_splits[u + 1] - row_splits[u] > kLongCornerList)
            long_list[atomicAdd(&long_list[v], 1)] = (int32_t)u;
}

// Rows in flight per walk step: kFilterWalk x (kAttrs + 1) x 3 doubles.
constexpr int kFilterWalk = 4;

// Smoothing.h:48-52 with TriangleMesh.cpp:336-342.
__device__ __forceinline__ double InverseDistance(const double a[3],
                                                  const double b[3]) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return 1.0 / (sqrt((dx * dx + dy * dy) + dz * dz) + 1e-12);
}

// The closing statement of a vertex with `cnt` neighbours.
template <int kKind>
__device__ __forceinline__ double FilterValue(double prev, double sum,
                                              double total, int cnt,
                                              double factor) {
    if (kKind == kFilterSharpen)
        return prev + factor * (prev * (double)cnt - sum);
    if (kKind == kFilterSimple) return (prev + sum) / (double)(1 + cnt);
    return total > 0.0 ? prev + factor * (sum / total - prev) : prev;
}

template <int kKind, int kAttrs>
__global__ void FilterThreadKernel(const int64_t* __restrict__ row_splits,
                                   const int32_t* __restrict__ neighbours,
                                   int64_t v, FilterPass f) {
    O3DMI_GRID_STRIDE(u, v) {
        const int64_t begin = row_splits[u];
        const int64_t size = row_splits[u + 1] - begin;
        if (size > kLongCornerList) continue;  // FilterWaveKernel's
        const int cnt = (int)size;
        const int32_t* list = neighbours + begin;
        double here[3] = {0, 0, 0};
        if (kKind == kFilterLaplacian)
            for (int c = 0; c < 3; ++c) here[c] = f.ref[3 * u + c];
        double sum[kAttrs][3], total = 0.0;
#pragma unroll
        for (int a = 0; a < kAttrs; ++a)
            sum[a][0] = sum[a][1] = sum[a][2] = 0.0;
        for (int j0 = 0; j0 < cnt; j0 += kFilterWalk) {
            double x[kFilterWalk][kAttrs][3], r[kFilterWalk][3];
#pragma unroll
            for (int j = 0; j < kFilterWalk; ++j) {
                if (j0 + j < cnt) {
                    const int64_t i = list[j0 + j];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (kKind == kFilterLaplacian)
                            r[j][c] = f.ref[3 * i + c];
#pragma unroll
                        for (int a = 0; a < kAttrs; ++a)
                            x[j][a][c] = f.prev[a][3 * i + c];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kFilterWalk; ++j) {
                if (j0 + j < cnt) {
                    double w = 1.0;
                    if (kKind == kFilterLaplacian) {
                        w = InverseDistance(here, r[j]);
                        total += w;
                    }
#pragma unroll
                    for (int a = 0; a < kAttrs; ++a)
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            sum[a][c] += kKind == kFilterLaplacian
                                                 ? w * x[j][a][c]
                                                 : x[j][a][c];
                }
            }
        }
#pragma unroll
        for (int a = 0; a < kAttrs; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                f.next[a][3 * u + c] = FilterValue<kKind>(
                        f.prev[a][3 * u + c], sum[a][c], total, cnt, f.factor);
    }
}

// A wave per listed vertex: 64 neighbours' rows are fetched at once, every
// lane forms its neighbour's weight and products, and they are added in list
// order (every lane does the same adds; lane 0 stores).
template <int kKind, int kAttrs>
__global__ void FilterWaveKernel(const int64_t* __restrict__ row_splits,
                                 const int32_t* __restrict__ neighbours,
                                 int64_t v, FilterPass f,
                                 const int32_t* __restrict__ long_list) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int n_long = long_list[v];
    for (int64_t w = wave; w < n_long; w += n_waves) {
        const int64_t u = long_list[w];
        const int64_t begin = row_splits[u];
        const int cnt = (int)(row_splits[u + 1] - begin);
        const int32_t* list = neighbours + begin;
        double here[3] = {0, 0, 0};
        if (kKind == kFilterLaplacian)
            for (int c = 0; c < 3; ++c) here[c] = f.ref[3 * u + c];
        double sum[kAttrs][3], total = 0.0;
#pragma unroll
        for (int a = 0; a < kAttrs; ++a)
            sum[a][0] = sum[a][1] = sum[a][2] = 0.0;
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            double x[kAttrs][3], weight = 0.0;
#pragma unroll
            for (int a = 0; a < kAttrs; ++a) x[a][0] = x[a][1] = x[a][2] = 0.0;
            if (j0 + lane < cnt) {
                const int64_t i = list[j0 + lane];
                if (kKind == kFilterLaplacian) {
                    const double r[3] = {f.ref[3 * i], f.ref[3 * i + 1],
                                         f.ref[3 * i + 2]};
                    weight = InverseDistance(here, r);
                }
#pragma unroll
                for (int a = 0; a < kAttrs; ++a)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double value = f.prev[a][3 * i + c];
                        x[a][c] = kKind == kFilterLaplacian ? weight * value
                                                            : value;
                    }
            }
            const int len = cnt - j0 < 64 ? cnt - j0 : 64;
            for (int l = 0; l < len; ++l) {
                if (kKind == kFilterLaplacian) total += __shfl(weight, l);
#pragma unroll
                for (int a = 0; a < kAttrs; ++a)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        sum[a][c] += __shfl(x[a][c], l);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < kAttrs; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    f.next[a][3 * u + c] = FilterValue<kKind>(
                            f.prev[a][3 * u + c], sum[a][c], total, cnt,
                            f.factor);
        }
    }
}

template <int kKind, int kAttrs>
int LaunchPass(const int64_t* row_splits_dev, const int32_t* neighbours_dev,
               int64_t v, const FilterPass& pass, const int32_t* long_list_dev,
               hipStream_t s) {
    O3DMI_LAUNCH((FilterThreadKernel<kKind, kAttrs>), v, row_splits_dev,
                 neighbours_dev, v, pass);
    hipLaunchKernelGGL((FilterWaveKernel<kKind, kAttrs>), WaveGrid(v),
                       dim3(kBlock), 0, s, row_splits_dev, neighbours_dev, v,
                       pass, long_list_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

template <int kKind>
int LaunchKind(const int64_t* row_splits_dev, const int32_t* neighbours_dev,
               int64_t v, const FilterPass& pass, const int32_t* long_list_dev,
               hipStream_t s) {
    switch (pass.n_attrs) {
        case 1:
            return LaunchPass<kKind, 1>(row_splits_dev, neighbours_dev, v, pass,
                                        long_list_dev, s);
        case 2:
            return LaunchPass<kKind, 2>(row_splits_dev, neighbours_dev, v, pass,
                                        long_list_dev, s);
        default:
            return LaunchPass<kKind, 3>(row_splits_dev, neighbours_dev, v, pass,
                                        long_list_dev, s);
    }
}

}  // namespace

int WidenAsync(const void* in_dev, int64_t n, int dtype, double* out_dev,
               hipStream_t s) {
    if (dtype == O3DMI_F64)
        O3DMI_LAUNCH(WidenKernel<double>, n, (const double*)in_dev, n, out_dev);
    else
        O3DMI_LAUNCH(WidenKernel<float>, n, (const float*)in_dev, n, out_dev);
    return O3DMI_OK;
}

int NarrowAsync(const double* in_dev, int64_t n, int dtype, void* out_dev,
                hipStream_t s) {
    if (dtype == O3DMI_F64)
        O3DMI_LAUNCH(NarrowKernel<double>, n, in_dev, n, (double*)out_dev);
    else
        O3DMI_LAUNCH(NarrowKernel<float>, n, in_dev, n, (float*)out_dev);
    return O3DMI_OK;
}

int LongListsAsync(const int64_t* row_splits_dev, int64_t v,
                   int32_t* long_list_dev, hipStream_t s) {
    O3DMI_LAUNCH(LongListsKernel, v, row_splits_dev, v, long_list_dev);
    return O3DMI_OK;
}

int FilterPassAsync(const int64_t* row_splits_dev,
                    const int32_t* neighbours_dev, int64_t v,
                    const FilterPass& pass, const int32_t* long_list_dev,
                    hipStream_t s) {
    O3DMI_REQUIRE(pass.n_attrs >= 1 && pass.n_attrs <= kMaxFilterAttrs,
                  "filter pass: 1 to 3 attributes");
    switch (pass.kind) {
        case kFilterSharpen:
            return LaunchKind<kFilterSharpen>(row_splits_dev, neighbours_dev, v,
                                              pass, long_list_dev, s);
        case kFilterSimple:
            return LaunchKind<kFilterSimple>(row_splits_dev, neighbours_dev, v,
                                             pass, long_list_dev, s);
        case kFilterLaplacian:
            return LaunchKind<kFilterLaplacian>(row_splits_dev, neighbours_dev,
                                                v, pass, long_list_dev, s);
    }
    SetLastError("filter pass: unknown kind");
    return O3DMI_ERR_INVALID_ARG;
}

}  // namespace o3dmi
