// PointCloud smoothing, boundary detection and normal orientation on MI355X:
//   SmoothLaplacian / SmoothTaubin  (t/geometry/kernel/PointCloudImpl.h:1357-1495)
//   SmoothMLS                       (:1504-1657)
//   SmoothBilateral                 (:1666-1753)
//   ComputeBoundaryPoints           (:355-506)
//   NormalizeNormals, OrientNormalsToAlignWithDirection,
//   OrientNormalsTowardsCameraLocation (:229-350)
// The per-point bodies are in pointcloud_smooth_device.h. This file holds the
// kernels that read a neighbour TABLE (fixed neighbourhoods, the radius-only
// MLS mode, the boundary seam) -- one wave per point, 64 entries of the row
// per step -- the three elementwise kernels, and the fused forms, where the
// search's own wave reduces the list it has just found: output policies of
// the searches of nns_wave.h.

#include "common.h"
#include "nns_wave.h"
#include "pointcloud_rows.h"
#include "pointcloud_smooth_device.h"

namespace o3dmi {
namespace {

constexpr int kTableBlock = 256;  // 4 waves = 4 points per workgroup

template <typename T>
struct LaplacianBody {
    LaplacianArgs<T> a;
    __device__ __forceinline__ void Run(int64_t i, const TableNb<T>& nb) const {
        LaplacianPoint(a, i, nb);
    }
};
template <typename T>
struct MlsBody {
    MlsArgs<T> a;
    __device__ __forceinline__ void Run(int64_t i, const TableNb<T>& nb) const {
        MlsPoint(a, i, nb);
    }
};
template <typename T>
struct BilateralBody {
    BilateralArgs<T> a;
    __device__ __forceinline__ void Run(int64_t i, const TableNb<T>& nb) const {
        BilateralPoint(a, i, nb);
    }
};
template <typename T>
struct BoundaryBody {
    BoundaryArgs<T> a;
    __device__ __forceinline__ void Run(int64_t i, const TableNb<T>& nb) const {
        BoundaryPoint(a, i, nb);
    }
};

// LaplacianOut / MlsOut / BilateralOut / BoundaryOut: the smoothed point (or
// the boundary flag) of query i straight from its list -- SmoothLaplacian /
// SmoothTaubin with re-searched neighbourhoods, SmoothMLS, SmoothBilateral,
// ComputeBoundaryPoints. Query i is point i of the cloud the index holds.
template <typename T>
struct LaplacianOut {
    LaplacianArgs<T> a;
    __device__ __forceinline__ void Write(const WaveTopK<T>& list,
                                          int64_t i) const {
        LaplacianPoint(a, i, ListOf(list));
    }
};
template <typename T>
struct MlsOut {
    MlsArgs<T> a;
    __device__ __forceinline__ void Write(const WaveTopK<T>& list,
                                          int64_t i) const {
        MlsPoint(a, i, ListOf(list));
    }
};
template <typename T>
struct BilateralOut {
    BilateralArgs<T> a;
    __device__ __forceinline__ void Write(const WaveTopK<T>& list,
                                          int64_t i) const {
        BilateralPoint(a, i, ListOf(list));
    }
};
template <typename T>
struct BoundaryOut {
    BoundaryArgs<T> a;
    __device__ __forceinline__ void Write(const WaveTopK<T>& list,
                                          int64_t i) const {
        BoundaryPoint(a, i, ListOf(list));
    }
};

// The float64 smoothing policies keep three coordinates and a weight per lane
// on top of the search's state: they get the register budget of three waves,
// so that nothing of theirs goes to scratch memory.
template <> struct KnnWaves<LaplacianOut<double>> {
    static constexpr int value = 3;
};
template <> struct KnnWaves<MlsOut<double>> { static constexpr int value = 3; };

template <typename T, typename Body>
__global__ void __launch_bounds__(kTableBlock)
TableSmoothKernel(const int32_t* __restrict__ indices,
                  const T* __restrict__ dist2,
                  const int32_t* __restrict__ counts,
                  const int64_t* __restrict__ row_splits, int64_t n, int width,
                  Body body) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wave; i < n; i += n_waves) {
        const int64_t offset = row_splits ? row_splits[i] : i * width;
        int count = row_splits ? (int)(row_splits[i + 1] - row_splits[i])
                               : (counts ? counts[i] : width);
        if (!row_splits && count > width) count = width;
        const TableNb<T> nb{indices + offset, dist2 ? dist2 + offset : nullptr,
                            count, n};
        body.Run(i, nb);
    }
}

__global__ void CountMaskKernel(const uint8_t* __restrict__ mask, int64_t n,
                                unsigned long long* __restrict__ count) {
    unsigned long long mine = 0;
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < n;
         w += (int64_t)gridDim.x * blockDim.x)
        mine += mask[w] != 0 ? 1 : 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mine += __shfl_xor(mine, s);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}

// NormalizeNormalsCPU, PointCloudImpl.h:229-259.
template <typename T>
__global__ void NormalizeNormalsKernel(T* __restrict__ ptr, int64_t n) {
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < n;
         w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t idx = 3 * w;
        T x = ptr[idx];
        T y = ptr[idx + 1];
        T z = ptr[idx + 2];
        const T norm = Sqrt(x * x + y * y + z * z);
        if (norm > 0) {
            x /= norm;
            y /= norm;
            z /= norm;
        }
        ptr[idx] = x;
        ptr[idx + 1] = y;
        ptr[idx + 2] = z;
    }
}

// OrientNormalsToAlignWithDirectionCPU, PointCloudImpl.h:261-295.
template <typename T>
__global__ void OrientToDirectionKernel(T* __restrict__ ptr, int64_t n, T dx,
                                        T dy, T dz) {
    const T direction_ptr[3] = {dx, dy, dz};
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < n;
         w += (int64_t)gridDim.x * blockDim.x) {
        T* normal = ptr + 3 * w;
        const T norm = Sqrt(normal[0] * normal[0] + normal[1] * normal[1] +
                            normal[2] * normal[2]);
        if (norm == 0.0) {
            normal[0] = direction_ptr[0];
            normal[1] = direction_ptr[1];
            normal[2] = direction_ptr[2];
        } else if (normal[0] * direction_ptr[0] + normal[1] * direction_ptr[1] +
                           normal[2] * direction_ptr[2] <
                   0) {
            normal[0] *= -1;
            normal[1] *= -1;
            normal[2] *= -1;
        }
    }
}

// OrientNormalsTowardsCameraLocationCPU, PointCloudImpl.h:297-351.
template <typename T>
__global__ void OrientToCameraKernel(const T* __restrict__ points_ptr,
                                     T* __restrict__ normals_ptr, int64_t n,
                                     T cx, T cy, T cz) {
    const T camera_ptr[3] = {cx, cy, cz};
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < n;
         w += (int64_t)gridDim.x * blockDim.x) {
        T* normal = normals_ptr + 3 * w;
        const T* point = points_ptr + 3 * w;
        const T reference[3] = {camera_ptr[0] - point[0],
                                camera_ptr[1] - point[1],
                                camera_ptr[2] - point[2]};
        const T norm = Sqrt(normal[0] * normal[0] + normal[1] * normal[1] +
                            normal[2] * normal[2]);
        if (norm == 0.0) {
            normal[0] = reference[0];
            normal[1] = reference[1];
            normal[2] = reference[2];
            const T norm_new =
                    Sqrt(normal[0] * normal[0] + normal[1] * normal[1] +
                         normal[2] * normal[2]);
            if (norm_new == 0.0) {
                normal[0] = 0.0;
                normal[1] = 0.0;
                normal[2] = 1.0;
            } else {
                normal[0] /= norm_new;
                normal[1] /= norm_new;
                normal[2] /= norm_new;
            }
        } else if (normal[0] * reference[0] + normal[1] * reference[1] +
                           normal[2] * reference[2] <
                   0) {
            normal[0] *= -1;
            normal[1] *= -1;
            normal[2] *= -1;
        }
    }
}

template <typename T>
int LaunchTable(const SmoothOp& op, const int32_t* indices, const void* dist2,
                const int32_t* counts, const int64_t* row_splits, int64_t n,
                int width, hipStream_t s) {
    const dim3 grid(GridFor(n, kTableBlock / 64, kCUs * 16)), block(kTableBlock);
    const T* d2 = (const T*)dist2;
    switch (op.kind) {
        case kSmoothLaplacian:
            hipLaunchKernelGGL((TableSmoothKernel<T, LaplacianBody<T>>), grid,
                               block, 0, s, indices, d2, counts, row_splits, n,
                               width,
                               LaplacianBody<T>{MakeLaplacianArgs<T>(op)});
            break;
        case kSmoothMls:
            hipLaunchKernelGGL((TableSmoothKernel<T, MlsBody<T>>), grid, block,
                               0, s, indices, d2, counts, row_splits, n, width,
                               MlsBody<T>{MakeMlsArgs<T>(op)});
            break;
        case kSmoothBilateral:
            hipLaunchKernelGGL((TableSmoothKernel<T, BilateralBody<T>>), grid,
                               block, 0, s, indices, d2, counts, row_splits, n,
                               width,
                               BilateralBody<T>{MakeBilateralArgs<T>(op)});
            break;
        case kSmoothBoundary:
            hipLaunchKernelGGL((TableSmoothKernel<T, BoundaryBody<T>>), grid,
                               block, 0, s, indices, d2, counts, row_splits, n,
                               width,
                               BoundaryBody<T>{MakeBoundaryArgs<T>(op)});
            break;
        default:
            SetLastError("smoothing: unknown operator");
            return O3DMI_ERR_INTERNAL;
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

template <typename T>
int LaunchHybridSmoothOp(const o3dmi_nns* nns, const void* points_dev,
                         int64_t n, int max_knn, const SmoothOp& op,
                         hipStream_t s) {
    const dim3 grid(GridFor(n, kCoopBlock / 64, kCUs * 16)), block(kCoopBlock);
    const size_t lds = CoopLdsBytesPerWave<T>() * (kCoopBlock / 64);
    const NnsView<T> nv = MakeView<T>(nns);
    const T* q = (const T*)points_dev;
    switch (op.kind) {
        case kSmoothMls:
            hipLaunchKernelGGL((HybridSearchKernel<T, MlsOut<T>>), grid, block,
                               lds, s, nv, q, n, max_knn,
                               MlsOut<T>{MakeMlsArgs<T>(op)});
            break;
        case kSmoothBilateral:
            hipLaunchKernelGGL((HybridSearchKernel<T, BilateralOut<T>>), grid,
                               block, lds, s, nv, q, n, max_knn,
                               BilateralOut<T>{MakeBilateralArgs<T>(op)});
            break;
        case kSmoothBoundary:
            hipLaunchKernelGGL((HybridSearchKernel<T, BoundaryOut<T>>), grid,
                               block, lds, s, nv, q, n, max_knn,
                               BoundaryOut<T>{MakeBoundaryArgs<T>(op)});
            break;
        default:
            SetLastError("hybrid search: unknown output policy");
            return O3DMI_ERR_INTERNAL;
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace

int HybridSearchSmoothOp(const o3dmi_nns* nns, const void* points_dev,
                         int64_t n, int max_knn, const SmoothOp& op,
                         hipStream_t s) {
    O3DMI_REQUIRE(nns != nullptr && points_dev != nullptr, "null argument");
    O3DMI_REQUIRE(max_knn >= 1 && max_knn <= kMaxKnn,
                  "max_knn must be in [1, 64]");
    if (n <= 0) return O3DMI_OK;
    return nns->dtype == O3DMI_F64
                   ? LaunchHybridSmoothOp<double>(nns, points_dev, n, max_knn,
                                                  op, s)
                   : LaunchHybridSmoothOp<float>(nns, points_dev, n, max_knn,
                                                 op, s);
}

int KnnSearchSmoothOp(const void* points_dev, int64_t n, int dtype, int knn,
                      const SmoothOp& op, hipStream_t s) {
    O3DMI_REQUIRE(op.kind == kSmoothLaplacian || op.kind == kSmoothMls,
                  "knn search: unknown output policy");
    const auto run = [&](auto make_out) {
        return KnnSearchRun(points_dev, n, points_dev, n, dtype, knn, make_out,
                            s);
    };
    if (op.kind == kSmoothLaplacian)
        return run([&](auto t) {
            return LaplacianOut<decltype(t)>{MakeLaplacianArgs<decltype(t)>(op)};
        });
    return run([&](auto t) {
        return MlsOut<decltype(t)>{MakeMlsArgs<decltype(t)>(op)};
    });
}

int TableSmoothOpAsync(const SmoothOp& op, const int32_t* indices_dev,
                       const void* dist2_dev, const int32_t* counts_dev,
                       const int64_t* row_splits_dev, int64_t n, int width,
                       int dtype, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    O3DMI_REQUIRE(indices_dev != nullptr, "null argument");
    O3DMI_REQUIRE(row_splits_dev || width >= 1, "bad table width");
    O3DMI_REQUIRE(op.kind != kSmoothBoundary ||
                          (!row_splits_dev && width <= kMaxSmoothNeighbors),
                  "boundary lists must be rows of at most 64 entries");
    return dtype == O3DMI_F64
                   ? LaunchTable<double>(op, indices_dev, dist2_dev, counts_dev,
                                         row_splits_dev, n, width, s)
                   : LaunchTable<float>(op, indices_dev, dist2_dev, counts_dev,
                                        row_splits_dev, n, width, s);
}

int CountMaskAsync(const uint8_t* mask_dev, int64_t n,
                   unsigned long long* count_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    int g = GridFor(n, kBlock);
    if (g > kCUs) g = kCUs;
    hipLaunchKernelGGL(CountMaskKernel, dim3(g), dim3(kBlock), 0, s, mask_dev,
                       n, count_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int NormalizeNormalsAsync(void* normals_dev, int64_t n, int dtype,
                          hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    const dim3 grid(GridFor(n, kBlock)), block(kBlock);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(NormalizeNormalsKernel<double>, grid, block, 0, s,
                           (double*)normals_dev, n);
    else
        hipLaunchKernelGGL(NormalizeNormalsKernel<float>, grid, block, 0, s,
                           (float*)normals_dev, n);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int OrientNormalsToDirectionAsync(void* normals_dev, int64_t n, int dtype,
                                  const double* vec3, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    const dim3 grid(GridFor(n, kBlock)), block(kBlock);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(OrientToDirectionKernel<double>, grid, block, 0, s,
                           (double*)normals_dev, n, vec3[0], vec3[1], vec3[2]);
    else
        hipLaunchKernelGGL(OrientToDirectionKernel<float>, grid, block, 0, s,
                           (float*)normals_dev, n, (float)vec3[0],
                           (float)vec3[1], (float)vec3[2]);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int OrientNormalsToCameraAsync(const void* points_dev, void* normals_dev,
                               int64_t n, int dtype, const double* vec3,
                               hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    const dim3 grid(GridFor(n, kBlock)), block(kBlock);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(OrientToCameraKernel<double>, grid, block, 0, s,
                           (const double*)points_dev, (double*)normals_dev, n,
                           vec3[0], vec3[1], vec3[2]);
    else
        hipLaunchKernelGGL(OrientToCameraKernel<float>, grid, block, 0, s,
                           (const float*)points_dev, (float*)normals_dev, n,
                           (float)vec3[0], (float)vec3[1], (float)vec3[2]);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace o3dmi
