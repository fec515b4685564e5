// Kernels behind PointCloud::FarthestPointDownSample, UniformDownSample,
// RandomDownSample, Crop and GetMinBound / GetMaxBound (t/geometry/
// PointCloud.cpp:569-648; t/geometry/kernel/PointCloudImpl.h:147-226).
//
//   farthest point   upstream runs six tensor ops and one host wait per
//                    sample. Here the sample loop is on the device, in one of
//                    two forms that give the same bits ((max value, min index)
//                    is associative and commutative):
//     resident       one workgroup of up to 512 threads, one launch for all samples: every thread
//                    keeps its points and their dist in registers; per sample
//                    the owner of the chosen point broadcasts it through LDS,
//                    every thread reduces its own (dist, index) pairs, a wave
//                    reduces by cross-lane moves, the waves meet in LDS: two
//                    workgroup barriers per sample, nothing else.
//     streamed       one launch per sample, enqueued back to back: dist lives
//                    in device memory, every workgroup updates a contiguous
//                    slice and leaves one (dist, index) partial, the workgroup
//                    that draws the last ticket reduces the partials and
//                    writes the next sample. No workgroup ever waits for
//                    another one.
//   uniform          a strided row copy of up to 8 attributes
//   random           indices[j] = SampleIndex(seed, n, j) (ransac.h); the rows
//                    go through the plain SelectByIndex gather
//   crop             one pass: compare, write the mask byte, count per wave
//   bounds           per-workgroup minima / maxima, then one workgroup
//
// Everything but the resident form is HBM-bound streaming.

#include "pointcloud_sample.h"

#include <limits>

#include "common.h"
#include "ransac.h"

namespace o3dmi {
namespace {

// ---- (max value, min index) ---------------------------------------------------
template <typename T>
__device__ __forceinline__ bool Better(T av, int ai, T bv, int bi) {
    return av > bv || (av == bv && ai < bi);
}

// The wave's best pair, in every lane.
template <typename T>
__device__ __forceinline__ void WaveBest(T& v, int& i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const T ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(i, m);
        if (Better(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
}

template <typename T>
__device__ __forceinline__ T SquaredDistance(T x, T y, T z, T qx, T qy, T qz) {
    const T dx = x - qx, dy = y - qy, dz = z - qz;
    return ((dx * dx) + dy * dy) + dz * dz;
}

// ---- farthest point, resident form ------------------------------------------
// 512 threads: eight waves of 256 registers fill the CU's register file; 1024
// threads of 128 registers would pay the fixed two dozen registers of a thread
// twice and hold a quarter fewer points.
constexpr int kResidentThreads = 512;
constexpr int kResidentWaves = kResidentThreads / 64;
// The most points per thread at which the kernel compiles without scratch
// (256 registers each; one more point spills. DESIGN.md has the counts).
constexpr int kResidentPerF32 = 60;
constexpr int kResidentPerF64 = 30;

// blockDim.x = 1 << shift threads; thread t holds points c * blockDim.x + t,
// c < kPer. A slot past n holds dist = -inf, which no update raises and no
// maximum picks (a real point has dist >= 0).
template <typename T, int kPer>
__global__ void __launch_bounds__(kResidentThreads)
FarthestResidentKernel(const T* __restrict__ p, int n, int64_t k, int start,
                       int shift, int64_t* __restrict__ order) {
    __shared__ T s_q[3];
    __shared__ T s_v[kResidentWaves];
    __shared__ int s_i[kResidentWaves];
    const int t = threadIdx.x;
    const int threads = 1 << shift;
    const int waves = threads >> 6;
    const T inf = std::numeric_limits<T>::infinity();

    T x[kPer], y[kPer], z[kPer], d[kPer];
#pragma unroll
    for (int c = 0; c < kPer; ++c) {
        const int j = c * threads + t;
        const bool in = j < n;
        x[c] = in ? p[3 * j + 0] : (T)0;
        y[c] = in ? p[3 * j + 1] : (T)0;
        z[c] = in ? p[3 * j + 2] : (T)0;
        d[c] = in ? inf : -inf;
    }

    int sel = start;
    for (int64_t i = 0;; ++i) {
        if (t == 0) order[i] = sel;
        if (i == k - 1) break;  // the last sample's arg-max is not needed
        // the owner of the chosen point broadcasts it
        if (t == (sel & (threads - 1))) {
            const int slot = sel >> shift;
            T qx = x[0], qy = y[0], qz = z[0];
#pragma unroll
            for (int c = 1; c < kPer; ++c)
                if (slot == c) {
                    qx = x[c];
                    qy = y[c];
                    qz = z[c];
                }
            s_q[0] = qx;
            s_q[1] = qy;
            s_q[2] = qz;
        }
        __syncthreads();
        const T qx = s_q[0], qy = s_q[1], qz = s_q[2];
        // own pairs: ascending index, so a strict > keeps the lowest
        T bv = -inf;
        int bc = 0;
#pragma unroll
        for (int c = 0; c < kPer; ++c) {
            const T dd = SquaredDistance(x[c], y[c], z[c], qx, qy, qz);
            d[c] = dd < d[c] ? dd : d[c];
            if (d[c] > bv) {
                bv = d[c];
                bc = c;
            }
        }
        int bi = bc * threads + t;
        WaveBest(bv, bi);
        if ((t & 63) == 0) {
            s_v[t >> 6] = bv;
            s_i[t >> 6] = bi;
        }
        __syncthreads();
        bv = s_v[0];
        bi = s_i[0];
        for (int w = 1; w < waves; ++w) {
            const T ov = s_v[w];
            const int oi = s_i[w];
            if (Better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        sel = bi < n ? bi : 0;  // bi >= n: a NaN cloud, which the driver refuses
    }
}

template <typename T, int kPer>
void LaunchResident(const void* p, int64_t n, int64_t k, int64_t start,
                    int shift, int64_t* order, hipStream_t s) {
    hipLaunchKernelGGL((FarthestResidentKernel<T, kPer>), dim3(1),
                       dim3(1 << shift), 0, s, (const T*)p, (int)n, k,
                       (int)start, shift, order);
}

// ---- farthest point, streamed form ------------------------------------------
constexpr int kStreamBlock = 256;
constexpr int kStreamMaxGrid = 1024;  // four workgroups per CU

// Scratch layout: dist {n} | partial values {kStreamMaxGrid} 64-bit |
// partial indices {kStreamMaxGrid} | the ticket.
struct StreamScratch {
    void* dist;
    unsigned long long* part_v;
    int* part_i;
    unsigned* ticket;
};

size_t DistBytes(int64_t n, int dtype) {
    const size_t b = (size_t)n * (dtype == O3DMI_F64 ? 8 : 4);
    return (b + 255) & ~(size_t)255;
}

StreamScratch CarveStream(void* scratch, int64_t n, int dtype) {
    StreamScratch w;
    char* at = (char*)scratch;
    w.dist = at;
    at += DistBytes(n, dtype);
    w.part_v = (unsigned long long*)at;
    at += sizeof(unsigned long long) * kStreamMaxGrid;
    w.part_i = (int*)at;
    at += sizeof(int) * kStreamMaxGrid;
    w.ticket = (unsigned*)at;
    return w;
}

__device__ __forceinline__ unsigned long long Bits(float v) {
    return (unsigned long long)__float_as_uint(v);
}
__device__ __forceinline__ unsigned long long Bits(double v) {
    return (unsigned long long)__double_as_longlong(v);
}
__device__ __forceinline__ void FromBits(unsigned long long b, float& v) {
    v = __uint_as_float((unsigned)b);
}
__device__ __forceinline__ void FromBits(unsigned long long b, double& v) {
    v = __longlong_as_double((long long)b);
}

// The workgroup's best pair, in thread 0.
template <typename T>
__device__ __forceinline__ void BlockBest(T& v, int& i, T* s_v, int* s_i) {
    WaveBest(v, i);
    if ((threadIdx.x & 63) == 0) {
        s_v[threadIdx.x >> 6] = v;
        s_i[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kStreamBlock / 64; ++w)
            if (Better(s_v[w], s_i[w], v, i)) {
                v = s_v[w];
                i = s_i[w];
            }
}

__global__ void FarthestStreamSetupKernel(int64_t start,
                                          int64_t* __restrict__ order,
                                          unsigned* __restrict__ ticket) {
    order[0] = start;
    *ticket = 0;
}

// Sample i -> i + 1: order_at = order + i holds the chosen index (written by
// the launch before); order_at[1] receives the next one. Workgroup b owns the
// points [b * slice, min(n, (b + 1) * slice)), never empty. The partials are
// handed over inside the launch: write-through stores, a fence, one atomic
// add; the workgroup that draws the last ticket fences and reads them with
// agent-scope loads. Nobody waits.
template <typename T>
__global__ void __launch_bounds__(kStreamBlock)
FarthestStreamKernel(const T* __restrict__ p, int n, int slice, int first,
                     T* __restrict__ dist, unsigned long long* part_v,
                     int* part_i, unsigned* ticket, int64_t* order_at) {
    __shared__ T s_v[kStreamBlock / 64];
    __shared__ int s_i[kStreamBlock / 64];
    __shared__ int s_last;
    const T inf = std::numeric_limits<T>::infinity();
    const int sel = (int)order_at[0];
    const T qx = p[3 * sel + 0], qy = p[3 * sel + 1], qz = p[3 * sel + 2];
    const int lo = blockIdx.x * slice;
    const int hi = lo + slice < n ? lo + slice : n;
    T bv = -inf;
    int bi = n;
    // unrolled: the loads of four strides are in flight together
#pragma unroll 4
    for (int j = lo + threadIdx.x; j < hi; j += kStreamBlock) {
        const T dd = SquaredDistance(p[3 * j + 0], p[3 * j + 1], p[3 * j + 2],
                                     qx, qy, qz);
        const T old = first ? inf : dist[j];
        const T nd = dd < old ? dd : old;
        dist[j] = nd;
        if (nd > bv) {  // ascending j: a strict > keeps the lowest index
            bv = nd;
            bi = j;
        }
    }
    BlockBest(bv, bi, s_v, s_i);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&part_v[blockIdx.x], Bits(bv), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part_i[blockIdx.x], bi, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const unsigned drawn = __hip_atomic_fetch_add(
                ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = drawn == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    bv = -inf;
    bi = n;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += kStreamBlock) {
        T ov;
        FromBits(__hip_atomic_load(&part_v[b], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT), ov);
        const int oi = __hip_atomic_load(&part_i[b], __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
        if (Better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    BlockBest(bv, bi, s_v, s_i);
    if (threadIdx.x == 0) {
        order_at[1] = bi < n ? bi : 0;  // bi >= n: see the resident form
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- masks ------------------------------------------------------------------
// GetPointMaskWithinAABB (PointCloudImpl.h:167-177).
template <typename T>
struct AabbPred {
    const T* p;
    T lo[3], hi[3];
    __device__ __forceinline__ bool operator()(int64_t i) const {
        const T x = p[3 * i + 0], y = p[3 * i + 1], z = p[3 * i + 2];
        return x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] &&
               z >= lo[2] && z <= hi[2];
    }
};

template <typename T>
__device__ __forceinline__ T AbsOf(T v) {
    return v < (T)0 ? -v : v;  // NaN stays NaN and fails the comparison
}

// GetPointMaskWithinOBB (PointCloudImpl.h:194-223); dot_3x1 adds left to right.
template <typename T>
struct ObbPred {
    const T* p;
    T center[3];
    T axis[3][3];  // axis[k] = column k of the rotation
    T half[3];
    __device__ __forceinline__ bool operator()(int64_t i) const {
        const T pd0 = p[3 * i + 0] - center[0];
        const T pd1 = p[3 * i + 1] - center[1];
        const T pd2 = p[3 * i + 2] - center[2];
        bool keep = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T dot = ((pd0 * axis[k][0]) + pd1 * axis[k][1]) +
                          pd2 * axis[k][2];
            keep = keep && AbsOf(dot) <= half[k];
        }
        return keep;
    }
};

// ---- uniform / random ---------------------------------------------------------
__global__ void StridedRowsKernel(int64_t m, int64_t every_k, SelectAttrs a,
                                  unsigned words) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < m;
         r += (int64_t)gridDim.x * blockDim.x)
        MoveRow(a, words, r * every_k, r);
}

__global__ void SampleIndicesKernel(uint64_t seed, int64_t n, int64_t m,
                                    int64_t* __restrict__ indices) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m;
         j += (int64_t)gridDim.x * blockDim.x)
        indices[j] = SampleIndex(seed, n, j);
}

// ---- bounds -------------------------------------------------------------------
constexpr int kBoundsMaxGrid = 1024;

// v[0..2] minima, v[3..5] maxima -> the workgroup's, in thread 0.
__device__ __forceinline__ void BlockMinMax(double v[6], double (*s)[6]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double o = __shfl_xor(v[k], m);
            if (k < 3 ? o < v[k] : o > v[k]) v[k] = o;
        }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 6; ++k) s[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kBlock / 64; ++w)
            for (int k = 0; k < 6; ++k) {
                const double o = s[w][k];
                if (k < 3 ? o < v[k] : o > v[k]) v[k] = o;
            }
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
MinMaxPartialKernel(const T* __restrict__ p, int64_t n,
                    double* __restrict__ partials) {
    __shared__ double s[kBlock / 64][6];
    const double inf = std::numeric_limits<double>::infinity();
    double v[6] = {inf, inf, inf, -inf, -inf, -inf};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double c = (double)p[3 * i + k];
            if (c < v[k]) v[k] = c;
            if (c > v[3 + k]) v[3 + k] = c;
        }
    BlockMinMax(v, s);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) partials[6 * blockIdx.x + k] = v[k];
}

__global__ void __launch_bounds__(kBlock)
MinMaxFinalKernel(const double* __restrict__ partials, int rows,
                  double* __restrict__ result) {
    __shared__ double s[kBlock / 64][6];
    const double inf = std::numeric_limits<double>::infinity();
    double v[6] = {inf, inf, inf, -inf, -inf, -inf};
    for (int r = threadIdx.x; r < rows; r += kBlock)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double o = partials[6 * r + k];
            if (k < 3 ? o < v[k] : o > v[k]) v[k] = o;
        }
    BlockMinMax(v, s);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) result[k] = v[k];
}

}  // namespace

// ---- launchers ----------------------------------------------------------------
int64_t FarthestResidentCapacity(int dtype) {
    if (dtype == O3DMI_F32) return (int64_t)kResidentPerF32 * kResidentThreads;
    if (dtype == O3DMI_F64) return (int64_t)kResidentPerF64 * kResidentThreads;
    return 0;
}

int FarthestOrderResidentAsync(const void* points_dev, int64_t n, int dtype,
                               int64_t k, int64_t start, int64_t* order_dev,
                               hipStream_t s) {
    if (k <= 0) return O3DMI_OK;
    O3DMI_REQUIRE(n >= 1 && n <= FarthestResidentCapacity(dtype),
                  "farthest point: cloud above the resident capacity");
    O3DMI_REQUIRE(k <= n && start >= 0 && start < n,
                  "farthest point: bad sample count or start");
    int shift = 6;  // whole waves, a power of two of threads
    while ((1 << shift) < kResidentThreads && (1ll << shift) < n) ++shift;
    const int64_t per = (n + (1ll << shift) - 1) >> shift;
#define O3DMI_RESIDENT(T, P)                                                   \
    if (per <= (P)) {                                                          \
        LaunchResident<T, (P)>(points_dev, n, k, start, shift, order_dev, s);  \
    } else
    if (dtype == O3DMI_F64) {
        O3DMI_RESIDENT(double, 1)
        O3DMI_RESIDENT(double, 2)
        O3DMI_RESIDENT(double, 4)
        O3DMI_RESIDENT(double, 8)
        O3DMI_RESIDENT(double, 16)
        LaunchResident<double, kResidentPerF64>(points_dev, n, k, start, shift,
                                                order_dev, s);
    } else {
        O3DMI_RESIDENT(float, 1)
        O3DMI_RESIDENT(float, 2)
        O3DMI_RESIDENT(float, 4)
        O3DMI_RESIDENT(float, 8)
        O3DMI_RESIDENT(float, 16)
        O3DMI_RESIDENT(float, 32)
        LaunchResident<float, kResidentPerF32>(points_dev, n, k, start, shift,
                                               order_dev, s);
    }
#undef O3DMI_RESIDENT
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int FarthestStreamGrid(int64_t n, int64_t* slice_out) {
    // whole workgroup strides per slice, at most kStreamMaxGrid slices
    int64_t slice = (n + kStreamMaxGrid - 1) / kStreamMaxGrid;
    slice = (slice + kStreamBlock - 1) / kStreamBlock * kStreamBlock;
    if (slice < kStreamBlock) slice = kStreamBlock;
    if (slice_out) *slice_out = slice;
    return (int)((n + slice - 1) / slice);
}

size_t FarthestStreamScratchBytes(int64_t n, int dtype) {
    return DistBytes(n, dtype) +
           (sizeof(unsigned long long) + sizeof(int)) * kStreamMaxGrid + 256;
}

int FarthestOrderStreamedAsync(const void* points_dev, int64_t n, int dtype,
                               int64_t k, int64_t start, int64_t* order_dev,
                               void* scratch_dev, hipStream_t s) {
    if (k <= 0) return O3DMI_OK;
    // indices, 3 * index and block * slice stay in int32
    O3DMI_REQUIRE(n >= 1 && n < (1ll << 27), "farthest point: n out of range");
    O3DMI_REQUIRE(k <= n && start >= 0 && start < n,
                  "farthest point: bad sample count or start");
    const StreamScratch w = CarveStream(scratch_dev, n, dtype);
    int64_t slice = 0;
    const int grid = FarthestStreamGrid(n, &slice);
    hipLaunchKernelGGL(FarthestStreamSetupKernel, dim3(1), dim3(1), 0, s, start,
                       order_dev, w.ticket);
    for (int64_t i = 0; i + 1 < k; ++i) {
        if (dtype == O3DMI_F64)
            hipLaunchKernelGGL(FarthestStreamKernel<double>, dim3(grid),
                               dim3(kStreamBlock), 0, s,
                               (const double*)points_dev, (int)n, (int)slice,
                               i == 0 ? 1 : 0, (double*)w.dist, w.part_v,
                               w.part_i, w.ticket, order_dev + i);
        else
            hipLaunchKernelGGL(FarthestStreamKernel<float>, dim3(grid),
                               dim3(kStreamBlock), 0, s,
                               (const float*)points_dev, (int)n, (int)slice,
                               i == 0 ? 1 : 0, (float*)w.dist, w.part_v,
                               w.part_i, w.ticket, order_dev + i);
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int StridedRowsAsync(int64_t m, int64_t every_k, const SelectAttrs& attrs,
                     hipStream_t s) {
    if (m <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(StridedRowsKernel, dim3(GridFor(m, kBlock)),
                       dim3(kBlock), 0, s, m, every_k, attrs, WordAttrs(attrs));
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SampleIndicesAsync(uint64_t seed, int64_t n, int64_t m,
                       int64_t* indices_dev, hipStream_t s) {
    if (m <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(SampleIndicesKernel, dim3(GridFor(m, kBlock)),
                       dim3(kBlock), 0, s, seed, n, m, indices_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

namespace {

template <typename T>
int LaunchAabb(const void* p, int64_t n, const double* lo, const double* hi,
               uint8_t* mask, unsigned long long* count, hipStream_t s) {
    AabbPred<T> box;
    box.p = (const T*)p;
    for (int k = 0; k < 3; ++k) {
        box.lo[k] = (T)lo[k];
        box.hi[k] = (T)hi[k];
    }
    return LaunchMask(n, box, mask, count, s);
}

template <typename T>
int LaunchObb(const void* p, int64_t n, const double* center,
              const double* rotation, const double* extent, uint8_t* mask,
              unsigned long long* count, hipStream_t s) {
    ObbPred<T> box;
    box.p = (const T*)p;
    for (int k = 0; k < 3; ++k) {
        box.center[k] = (T)center[k];
        box.half[k] = (T)extent[k] / (T)2;
        for (int r = 0; r < 3; ++r) box.axis[k][r] = (T)rotation[3 * r + k];
    }
    return LaunchMask(n, box, mask, count, s);
}

}  // namespace

int AabbMaskAsync(const void* points_dev, int64_t n, int dtype,
                  const double min_bound[3], const double max_bound[3],
                  uint8_t* mask_dev, unsigned long long* count_dev,
                  hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    return dtype == O3DMI_F64
                   ? LaunchAabb<double>(points_dev, n, min_bound, max_bound,
                                        mask_dev, count_dev, s)
                   : LaunchAabb<float>(points_dev, n, min_bound, max_bound,
                                       mask_dev, count_dev, s);
}

int ObbMaskAsync(const void* points_dev, int64_t n, int dtype,
                 const double center[3], const double rotation[9],
                 const double extent[3], uint8_t* mask_dev,
                 unsigned long long* count_dev, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    return dtype == O3DMI_F64
                   ? LaunchObb<double>(points_dev, n, center, rotation, extent,
                                       mask_dev, count_dev, s)
                   : LaunchObb<float>(points_dev, n, center, rotation, extent,
                                      mask_dev, count_dev, s);
}

size_t MinMaxScratchDoubles() { return 6 * (size_t)kBoundsMaxGrid + 8; }

int MinMaxBoundAsync(const void* points_dev, int64_t n, int dtype,
                     double* scratch_dev, double** result_dev, hipStream_t s) {
    O3DMI_REQUIRE(n >= 1, "bounds: empty cloud");
    double* partials = scratch_dev;
    double* result = scratch_dev + 6 * (size_t)kBoundsMaxGrid;
    const int rows = GridFor(n, kBlock, kBoundsMaxGrid);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(MinMaxPartialKernel<double>, dim3(rows),
                           dim3(kBlock), 0, s, (const double*)points_dev, n,
                           partials);
    else
        hipLaunchKernelGGL(MinMaxPartialKernel<float>, dim3(rows), dim3(kBlock),
                           0, s, (const float*)points_dev, n, partials);
    hipLaunchKernelGGL(MinMaxFinalKernel, dim3(1), dim3(kBlock), 0, s, partials,
                       rows, result);
    O3DMI_HIP_CHECK(hipGetLastError());
    *result_dev = result;
    return O3DMI_OK;
}

}  // namespace o3dmi
