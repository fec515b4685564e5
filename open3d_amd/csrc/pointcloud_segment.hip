// Elementwise kernels of PointCloud::ClusterDBSCAN and the kernels of
// PointCloud::SegmentPlane (legacy geometry/PointCloudCluster.cpp,
// geometry/PointCloudSegmentation.cpp; the tensor class converts to the legacy
// cloud and calls them, t/geometry/PointCloud.cpp:1634-1666).
//
//   DBSCAN        identity, flatten (pointer jump + root flags); the two
//                 neighbourhood sweeps are wave-per-point kernels: sinks of
//                 the 27-cell gather of nns_wave.h
//   hypotheses    one thread per RANSAC iteration: sample -> plane, float64
//   score         lane = hypothesis, plane in registers; the workgroup walks a
//                 tile of points that is the same for every lane, so the point
//                 loads are scalar and no cross-lane reduction exists; one
//                 partial per (hypothesis, tile), summed in tile order by a
//                 second launch
//   final         inlier flags -> PrefixSumAsync -> ascending indices; the
//                 refit's centroid and centred sums as per-workgroup partials
//
// Every float64 expression here is evaluated as written: the library is built
// with -ffp-contract=off, restated below for this file.
#pragma clang fp contract(off)

#include "pointcloud_segment.h"

#include "common.h"
#include "nns_wave.h"
#include "union_find.h"

namespace o3dmi {
namespace {

__global__ void IdentityKernel(int* __restrict__ parent, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
        parent[i] = (int)i;
}

// parent[] is final here (the union sweep was an earlier launch) and a
// non-root's parent is a smaller index, so the walk ends.
__global__ void FlattenKernel(const int* __restrict__ parent,
                              const int* __restrict__ counts, int need,
                              int64_t n, int* __restrict__ root,
                              int* __restrict__ is_root) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        int r = -1;
        if (counts[i] >= need) {
            r = (int)i;
            for (int p = parent[r]; p != r; p = parent[r]) r = p;
        }
        root[i] = r;
        is_root[i] = r == (int)i ? 1 : 0;
    }
}

// ---- ClusterDBSCAN's two sweeps ------------------------------------------------
// Point j is a core point when counts[j] >= need. parent[] is a forest over
// the core points in which a non-root's parent is always a SMALLER index:
// a root is only ever hooked under a smaller root, with one CAS, so the root
// of a finished tree is the lowest core index of its component whatever order
// the waves ran in.

// DbscanFind / DbscanUnite: union_find.h.

struct UnionSink {
    const int* counts;
    int* parent;
    int need;
    int self;
    template <typename T>
    __device__ __forceinline__ void Push(T, int j, T, T, T) {
        if (j != kNoIndex && j < self && counts[j] >= need)
            DbscanUnite(parent, self, j);
    }
};

template <typename T>
__global__ void __launch_bounds__(kCoopBlock)
DbscanUnionKernel(NnsView<T> nv, const T* __restrict__ q, int64_t nq,
                  const int* __restrict__ counts, int need,
                  int* __restrict__ parent) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wave; i < nq; i += n_waves) {
        if (counts[i] < need) continue;  // wave-uniform
        const T qq[3] = {q[3 * i + 0], q[3 * i + 1], q[3 * i + 2]};
        long long cx, cy, cz;
        CellOf(qq, nv.inv_cell, cx, cy, cz);
        UnionSink sink = {counts, parent, need, (int)i};
        O3DMI_GATHER_BALL(T, nv, qq, cx, cy, cz, sink);
    }
}

// The smallest cluster label among a lane's core candidates.
struct MinLabelSink {
    const int* counts;
    const int* root;
    const int64_t* cluster;
    int need;
    int best;
    template <typename T>
    __device__ __forceinline__ void Push(T, int j, T, T, T) {
        if (j != kNoIndex && counts[j] >= need) {
            const int l = (int)cluster[root[j]];
            best = l < best ? l : best;
        }
    }
};

template <typename T>
__global__ void __launch_bounds__(kCoopBlock)
DbscanLabelKernel(NnsView<T> nv, const T* __restrict__ q, int64_t nq,
                  const int* __restrict__ counts, int need,
                  const int* __restrict__ root,
                  const int64_t* __restrict__ cluster, int* __restrict__ labels,
                  unsigned long long* __restrict__ noise) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long n_noise = 0;  // wave-uniform
    for (int64_t i = wave; i < nq; i += n_waves) {
        const int c = counts[i];
        int label = -1;
        if (c >= need) {
            label = (int)cluster[root[i]];
        } else if (c > 1) {  // somebody besides the point itself is in range
            const T qq[3] = {q[3 * i + 0], q[3 * i + 1], q[3 * i + 2]};
            long long cx, cy, cz;
            CellOf(qq, nv.inv_cell, cx, cy, cz);
            MinLabelSink sink = {counts, root, cluster, need, kNoIndex};
            O3DMI_GATHER_BALL(T, nv, qq, cx, cy, cz, sink);
            int m = sink.best;
            O3DMI_WAVE_MIN(m);
            label = m == kNoIndex ? -1 : m;
        }
        if ((threadIdx.x & 63) == 0) labels[i] = label;
        n_noise += label < 0 ? 1 : 0;
    }
    if ((threadIdx.x & 63) == 0 && n_noise) atomicAdd(noise, n_noise);
}

// ---- SegmentPlane ------------------------------------------------------------

struct Vec3d {
    double x, y, z;
};

template <typename T>
__device__ __forceinline__ Vec3d LoadPoint(const T* __restrict__ pts,
                                           int64_t i) {
    return {(double)pts[3 * i + 0], (double)pts[3 * i + 1],
            (double)pts[3 * i + 2]};
}

// abc / |abc| and d = -abc . p; false (zero plane) when |abc| == 0.
__device__ __forceinline__ bool FinishPlane(Vec3d abc, const Vec3d& p,
                                            double* plane) {
    const double norm = sqrt((abc.x * abc.x + abc.y * abc.y) + abc.z * abc.z);
    if (norm == 0) {
        plane[0] = plane[1] = plane[2] = plane[3] = 0;
        return false;
    }
    abc.x /= norm;
    abc.y /= norm;
    abc.z /= norm;
    plane[0] = abc.x;
    plane[1] = abc.y;
    plane[2] = abc.z;
    plane[3] = -((abc.x * p.x + abc.y * p.y) + abc.z * p.z);
    return true;
}

template <typename T>
__global__ void PlaneHypothesesKernel(const T* __restrict__ pts, int64_t n,
                                      uint64_t seed, int64_t first,
                                      int64_t count, int ransac_n,
                                      double* __restrict__ planes,
                                      int* __restrict__ valid) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    int64_t pick[kPlaneMaxN];
    PlaneSample(seed, first + k, ransac_n, n, pick);
    double plane[4];
    bool ok;
    if (ransac_n == 3) {
        // TriangleMesh::ComputeTrianglePlane
        const Vec3d p0 = LoadPoint(pts, pick[0]), p1 = LoadPoint(pts, pick[1]),
                    p2 = LoadPoint(pts, pick[2]);
        const Vec3d e0 = {p1.x - p0.x, p1.y - p0.y, p1.z - p0.z};
        const Vec3d e1 = {p2.x - p0.x, p2.y - p0.y, p2.z - p0.z};
        const Vec3d abc = {e0.y * e1.z - e0.z * e1.y, e0.z * e1.x - e0.x * e1.z,
                           e0.x * e1.y - e0.y * e1.x};
        ok = FinishPlane(abc, p0, plane);
    } else {
        Vec3d c = {0, 0, 0};
        for (int j = 0; j < ransac_n; ++j) {
            const Vec3d p = LoadPoint(pts, pick[j]);
            c.x += p.x;
            c.y += p.y;
            c.z += p.z;
        }
        const double m = (double)ransac_n;
        c.x /= m;
        c.y /= m;
        c.z /= m;
        double sums[6] = {0, 0, 0, 0, 0, 0};
        for (int j = 0; j < ransac_n; ++j) {
            const Vec3d p = LoadPoint(pts, pick[j]);
            const double rx = p.x - c.x, ry = p.y - c.y, rz = p.z - c.z;
            sums[0] += rx * rx;
            sums[1] += rx * ry;
            sums[2] += rx * rz;
            sums[3] += ry * ry;
            sums[4] += ry * rz;
            sums[5] += rz * rz;
        }
        double abc[3];
        PlaneNormalFromSums(sums, abc);
        ok = FinishPlane({abc[0], abc[1], abc[2]}, c, plane);
    }
    for (int j = 0; j < 4; ++j) planes[4 * k + j] = plane[j];
    valid[k] = ok ? 1 : 0;
}

__device__ __forceinline__ double PlaneDistance(double a, double b, double c,
                                                double d, double x, double y,
                                                double z) {
    return fabs(((a * x + b * y) + c * z) + d);
}

// grid (tiles, ceil(b / kPlaneBlock)). The point index j is the same in every
// lane: the three coordinate loads are scalar.
template <typename T>
__global__ void __launch_bounds__(kPlaneBlock)
PlaneScoreKernel(const T* __restrict__ pts, int64_t n,
                 const double* __restrict__ planes, int b, double threshold,
                 int* __restrict__ part_counts,
                 double* __restrict__ part_sums) {
    const int h = blockIdx.y * kPlaneBlock + threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int hc = h < b ? h : b - 1;
    const double pa = planes[4 * hc + 0], pb = planes[4 * hc + 1],
                 pc = planes[4 * hc + 2], pd = planes[4 * hc + 3];
    const int64_t j0 = tile * kPlaneTile;
    const int64_t j1 = j0 + kPlaneTile < n ? j0 + kPlaneTile : n;
    int count = 0;
    double sum = 0;
#pragma unroll 4
    for (int64_t j = j0; j < j1; ++j) {
        const double x = (double)pts[3 * j + 0], y = (double)pts[3 * j + 1],
                     z = (double)pts[3 * j + 2];
        const double dist = PlaneDistance(pa, pb, pc, pd, x, y, z);
        const bool in = dist < threshold;
        count += in ? 1 : 0;
        sum += in ? dist * dist : 0.0;
    }
    if (h < b) {
        part_counts[tile * b + h] = count;
        part_sums[tile * b + h] = sum;
    }
}

__global__ void PlaneScoreSumKernel(const int* __restrict__ part_counts,
                                    const double* __restrict__ part_sums,
                                    int64_t tiles, int b,
                                    int64_t* __restrict__ counts,
                                    double* __restrict__ sums) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= b) return;
    int64_t count = 0;
    double sum = 0;
    for (int64_t t = 0; t < tiles; ++t) {
        count += part_counts[t * b + h];
        sum += part_sums[t * b + h];
    }
    counts[h] = count;
    sums[h] = sum;
}

struct Plane4 {
    double a, b, c, d;
};

template <typename T>
__global__ void PlaneFlagsKernel(const T* __restrict__ pts, int64_t n,
                                 Plane4 p, double threshold,
                                 int* __restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const Vec3d q = LoadPoint(pts, i);
        flags[i] = PlaneDistance(p.a, p.b, p.c, p.d, q.x, q.y, q.z) < threshold
                           ? 1
                           : 0;
    }
}

__global__ void PlaneIndicesKernel(const int* __restrict__ flags,
                                   const int64_t* __restrict__ position,
                                   int64_t n, int64_t* __restrict__ indices) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
        if (flags[i]) indices[position[i]] = i;
}

// One workgroup per kRefitTile inliers; row blockIdx.x of `partials` {.,8}.
template <typename T, bool CENTRED>
__global__ void __launch_bounds__(kBlock)
PlaneRefitKernel(const T* __restrict__ pts, const int64_t* __restrict__ indices,
                 int64_t m, Vec3d centroid, double* __restrict__ partials) {
    constexpr int kTerms = CENTRED ? 6 : 3;
    __shared__ double lds[kTerms][kBlock];
    const int64_t r0 = (int64_t)blockIdx.x * kRefitTile;
    const int64_t r1 = r0 + kRefitTile < m ? r0 + kRefitTile : m;
    double acc[kTerms];
    for (int k = 0; k < kTerms; ++k) acc[k] = 0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
        const Vec3d p = LoadPoint(pts, indices[r]);
        if constexpr (CENTRED) {
            const double rx = p.x - centroid.x, ry = p.y - centroid.y,
                         rz = p.z - centroid.z;
            acc[0] += rx * rx;
            acc[1] += rx * ry;
            acc[2] += rx * rz;
            acc[3] += ry * ry;
            acc[4] += ry * rz;
            acc[5] += rz * rz;
        } else {
            acc[0] += p.x;
            acc[1] += p.y;
            acc[2] += p.z;
        }
    }
    for (int k = 0; k < kTerms; ++k) lds[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int k = 0; k < kTerms; ++k)
                lds[k][threadIdx.x] += lds[k][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x < kTerms)
        partials[8 * (int64_t)blockIdx.x + threadIdx.x] = lds[threadIdx.x][0];
}

}  // namespace

int DbscanIdentityAsync(int32_t* parent_dev, int64_t n, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(IdentityKernel, dim3(GridFor(n, kBlock)), dim3(kBlock),
                       0, s, parent_dev, n);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int DbscanUnionSweep(const o3dmi_nns* nns, const void* points_dev, int64_t n,
                     const int32_t* counts_dev, int need, int32_t* parent_dev,
                     hipStream_t s) {
    O3DMI_REQUIRE(nns && points_dev && counts_dev && parent_dev,
                  "null argument");
    if (n <= 0) return O3DMI_OK;
    const dim3 grid(GridFor(n, kCoopBlock / 64, kCUs * 16)), block(kCoopBlock);
    if (nns->dtype == O3DMI_F64)
        hipLaunchKernelGGL(DbscanUnionKernel<double>, grid, block, 0, s,
                           MakeView<double>(nns), (const double*)points_dev, n,
                           counts_dev, need, parent_dev);
    else
        hipLaunchKernelGGL(DbscanUnionKernel<float>, grid, block, 0, s,
                           MakeView<float>(nns), (const float*)points_dev, n,
                           counts_dev, need, parent_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int DbscanLabelSweep(const o3dmi_nns* nns, const void* points_dev, int64_t n,
                     const int32_t* counts_dev, int need,
                     const int32_t* root_dev, const int64_t* cluster_dev,
                     int32_t* labels_dev, unsigned long long* noise_dev,
                     hipStream_t s) {
    O3DMI_REQUIRE(nns && points_dev && counts_dev && root_dev && cluster_dev &&
                          labels_dev && noise_dev,
                  "null argument");
    if (n <= 0) return O3DMI_OK;
    const dim3 grid(GridFor(n, kCoopBlock / 64, kCUs * 16)), block(kCoopBlock);
    if (nns->dtype == O3DMI_F64)
        hipLaunchKernelGGL(DbscanLabelKernel<double>, grid, block, 0, s,
                           MakeView<double>(nns), (const double*)points_dev, n,
                           counts_dev, need, root_dev, cluster_dev, labels_dev,
                           noise_dev);
    else
        hipLaunchKernelGGL(DbscanLabelKernel<float>, grid, block, 0, s,
                           MakeView<float>(nns), (const float*)points_dev, n,
                           counts_dev, need, root_dev, cluster_dev, labels_dev,
                           noise_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int DbscanFlattenAsync(const int32_t* parent_dev, const int32_t* counts_dev,
                       int need, int64_t n, int32_t* root_dev,
                       int32_t* is_root_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(FlattenKernel, dim3(GridFor(n, kBlock)), dim3(kBlock), 0,
                       s, parent_dev, counts_dev, need, n, root_dev,
                       is_root_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int PlaneHypothesesAsync(const void* points_dev, int64_t n, int dtype,
                         uint64_t seed, int64_t first, int64_t count,
                         int ransac_n, double* planes_dev, int32_t* valid_dev,
                         hipStream_t s) {
    if (count <= 0) return O3DMI_OK;
    const dim3 grid((unsigned)((count + kBlock - 1) / kBlock)), block(kBlock);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(PlaneHypothesesKernel<double>, grid, block, 0, s,
                           (const double*)points_dev, n, seed, first, count,
                           ransac_n, planes_dev, valid_dev);
    else
        hipLaunchKernelGGL(PlaneHypothesesKernel<float>, grid, block, 0, s,
                           (const float*)points_dev, n, seed, first, count,
                           ransac_n, planes_dev, valid_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int PlaneScoreAsync(const void* points_dev, int64_t n, int dtype,
                    const double* planes_dev, int64_t b, double threshold,
                    int32_t* part_counts_dev, double* part_sums_dev,
                    int64_t* counts_dev, double* d2_sums_dev, hipStream_t s) {
    if (b <= 0) return O3DMI_OK;
    O3DMI_REQUIRE(b <= PlaneBatchCap(n), "plane score: batch above the cap");
    const int64_t tiles = PlaneTiles(n);
    if (tiles > 0) {
        const dim3 grid((unsigned)tiles,
                        (unsigned)((b + kPlaneBlock - 1) / kPlaneBlock)),
                block(kPlaneBlock);
        if (dtype == O3DMI_F64)
            hipLaunchKernelGGL(PlaneScoreKernel<double>, grid, block, 0, s,
                               (const double*)points_dev, n, planes_dev,
                               (int)b, threshold, part_counts_dev,
                               part_sums_dev);
        else
            hipLaunchKernelGGL(PlaneScoreKernel<float>, grid, block, 0, s,
                               (const float*)points_dev, n, planes_dev, (int)b,
                               threshold, part_counts_dev, part_sums_dev);
    }
    hipLaunchKernelGGL(PlaneScoreSumKernel,
                       dim3((unsigned)((b + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, s, part_counts_dev, part_sums_dev,
                       tiles, (int)b, counts_dev, d2_sums_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int PlaneInlierFlagsAsync(const void* points_dev, int64_t n, int dtype,
                          const double plane[4], double threshold,
                          int32_t* flags_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    const Plane4 p = {plane[0], plane[1], plane[2], plane[3]};
    const dim3 grid(GridFor(n, kBlock)), block(kBlock);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(PlaneFlagsKernel<double>, grid, block, 0, s,
                           (const double*)points_dev, n, p, threshold,
                           flags_dev);
    else
        hipLaunchKernelGGL(PlaneFlagsKernel<float>, grid, block, 0, s,
                           (const float*)points_dev, n, p, threshold,
                           flags_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int PlaneInlierIndicesAsync(const int32_t* flags_dev,
                            const int64_t* position_dev, int64_t n,
                            int64_t* indices_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(PlaneIndicesKernel, dim3(GridFor(n, kBlock)),
                       dim3(kBlock), 0, s, flags_dev, position_dev, n,
                       indices_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int PlaneRefitSumsAsync(const void* points_dev, int dtype,
                        const int64_t* indices_dev, int64_t m, int centred,
                        const double centroid[3], double* partials_dev,
                        hipStream_t s) {
    if (m <= 0) return O3DMI_OK;
    const dim3 grid((unsigned)RefitBlocks(m)), block(kBlock);
    const Vec3d c = {centroid[0], centroid[1], centroid[2]};
    if (dtype == O3DMI_F64) {
        if (centred)
            hipLaunchKernelGGL((PlaneRefitKernel<double, true>), grid, block, 0,
                               s, (const double*)points_dev, indices_dev, m, c,
                               partials_dev);
        else
            hipLaunchKernelGGL((PlaneRefitKernel<double, false>), grid, block,
                               0, s, (const double*)points_dev, indices_dev, m,
                               c, partials_dev);
    } else {
        if (centred)
            hipLaunchKernelGGL((PlaneRefitKernel<float, true>), grid, block, 0,
                               s, (const float*)points_dev, indices_dev, m, c,
                               partials_dev);
        else
            hipLaunchKernelGGL((PlaneRefitKernel<float, false>), grid, block, 0,
                               s, (const float*)points_dev, indices_dev, m, c,
                               partials_dev);
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace o3dmi
