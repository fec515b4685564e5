// Per-point bodies of the PointCloud smoothing and boundary kernels: one wave
// serves one point. They are shared by the output policies of the searches
// (the neighbour list is in the wave's lanes when the search ends) and by the
// table-reading kernels, both in pointcloud_smooth.hip, so both forms run the
// same statements in the same order.
//
// A neighbour source `Nb` hands lane l entry base + l of the point's list:
//   int count                             entries of the list (wave-uniform)
//   void Load(int base, int& idx, T& d2)  idx < 0: no entry
// Sums run over the entries in list order: lane j's term is read into scalar
// registers (WaveRead) and added as the j-th term, in the point dtype, in upstream's
// expressions (t/geometry/kernel/PointCloudImpl.h:355-506, 1357-1753).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "eigen3.h"
#include "pointcloud_smooth.h"

namespace o3dmi {

__device__ __forceinline__ float ExpOf(float v) { return expf(v); }
__device__ __forceinline__ double ExpOf(double v) { return exp(v); }
__device__ __forceinline__ float Atan2Of(float y, float x) {
    return atan2f(y, x);
}
__device__ __forceinline__ double Atan2Of(double y, double x) {
    return atan2(y, x);
}

// Lane j's value on every lane, j wave-uniform: a v_readlane into a scalar
// register (a __shfl would go through the LDS crossbar for the same bits).
__device__ __forceinline__ float WaveRead(float v, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}
__device__ __forceinline__ double WaveRead(double v, int j) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, j);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), j);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <typename T>
struct LaplacianArgs {
    const T* pts;
    T* out;
    T alpha;
};
template <typename T>
struct MlsArgs {
    const T* pts;
    T* out;      // holds a copy of pts
    T* normals;  // in / out (a copy of the incoming normals), or NULL
    T inv_radius2;
};
template <typename T>
struct BilateralArgs {
    const T* pts;
    const T* normals;
    T* out;  // holds a copy of pts
    T inv_sigma_s2, inv_sigma_r2;
};
template <typename T>
struct BoundaryArgs {
    const T* pts;
    const T* normals;
    uint8_t* mask;  // zeroed by the caller
    double threshold_rad;
};

template <typename T>
inline LaplacianArgs<T> MakeLaplacianArgs(const SmoothOp& op) {
    return {(const T*)op.points, (T*)op.out_points, static_cast<T>(op.p0)};
}
template <typename T>
inline MlsArgs<T> MakeMlsArgs(const SmoothOp& op) {
    const double radius = op.p0;
    return {(const T*)op.points, (T*)op.out_points, (T*)op.out_normals,
            radius > 0.0 ? static_cast<T>(1.0 / (radius * radius))
                         : static_cast<T>(0.0)};
}
template <typename T>
inline BilateralArgs<T> MakeBilateralArgs(const SmoothOp& op) {
    return {(const T*)op.points, (const T*)op.normals, (T*)op.out_points,
            static_cast<T>(1.0 / (2.0 * op.p0 * op.p0)),
            static_cast<T>(1.0 / (2.0 * op.p1 * op.p1))};
}
template <typename T>
inline BoundaryArgs<T> MakeBoundaryArgs(const SmoothOp& op) {
    return {(const T*)op.points, (const T*)op.normals, op.mask,
            op.p0 * M_PI / 180.0};
}

// Rows of a neighbour table (fixed width or CSR) as a neighbour source.
template <typename T>
struct TableNb {
    const int32_t* idx;
    const T* d2;  // NULL: every distance is 0
    int count;
    int64_t n_points;  // an index outside [0, n_points) is no entry
    __device__ __forceinline__ void Load(int base, int& i, T& d) const {
        const int j = base + (int)(threadIdx.x & 63);
        i = j < count ? idx[j] : -1;
        if ((int64_t)i >= n_points) i = -1;
        d = (d2 && j < count) ? d2[j] : T(0);
    }
};

// ApplyLaplacianPass, PointCloudImpl.h:1357-1406.
template <typename T, typename Nb>
__device__ __forceinline__ void LaplacianPoint(const LaplacianArgs<T>& a,
                                               int64_t i, const Nb& nb) {
    T mean[3] = {0, 0, 0};
    int32_t count = 0;
    for (int base = 0; base < nb.count; base += 64) {
        int ni;
        T nd;
        nb.Load(base, ni, nd);
        const bool ok = ni >= 0 && (int64_t)ni != i;
        T x = T(0), y = T(0), z = T(0);
        if (ok) {
            x = a.pts[3 * (int64_t)ni + 0];
            y = a.pts[3 * (int64_t)ni + 1];
            z = a.pts[3 * (int64_t)ni + 2];
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
        const int lim = nb.count - base < 64 ? nb.count - base : 64;
        for (int j = 0; j < lim; ++j) {
            const T sx = WaveRead(x, j), sy = WaveRead(y, j), sz = WaveRead(z, j);
            if ((m >> j) & 1ull) {
                mean[0] += sx;
                mean[1] += sy;
                mean[2] += sz;
                ++count;
            }
        }
    }
    if ((threadIdx.x & 63) != 0) return;
    const int64_t offset = 3 * i;
    if (count == 0) {
        a.out[offset + 0] = a.pts[offset + 0];
        a.out[offset + 1] = a.pts[offset + 1];
        a.out[offset + 2] = a.pts[offset + 2];
        return;
    }
    const T inv_count = static_cast<T>(1.0 / count);
    a.out[offset + 0] = a.pts[offset + 0] +
                        a.alpha * (mean[0] * inv_count - a.pts[offset + 0]);
    a.out[offset + 1] = a.pts[offset + 1] +
                        a.alpha * (mean[1] * inv_count - a.pts[offset + 1]);
    a.out[offset + 2] = a.pts[offset + 2] +
                        a.alpha * (mean[2] * inv_count - a.pts[offset + 2]);
}

// SmoothMLS' per-point body, PointCloudImpl.h:1560-1655. The normal is this
// code base's SmallestEigenvectorSym3 (eigen3.h), not upstream's closed form.
template <typename T, typename Nb>
__device__ __forceinline__ void MlsPoint(const MlsArgs<T>& a, int64_t i,
                                         const Nb& nb) {
    const bool writer = (threadIdx.x & 63) == 0;
    const int64_t po = 3 * i;
    if (nb.count < 3) {
        if (a.normals && writer) {
            T* normal = a.normals + po;
            const T norm = Sqrt(normal[0] * normal[0] + normal[1] * normal[1] +
                                normal[2] * normal[2]);
            if (norm > 0) {
                normal[0] /= norm;
                normal[1] /= norm;
                normal[2] /= norm;
            }
        }
        return;
    }
    T centroid[3] = {0, 0, 0};
    T weight_sum = 0;
    for (int base = 0; base < nb.count; base += 64) {
        int ni;
        T nd;
        nb.Load(base, ni, nd);
        const bool ok = ni >= 0;
        T w = T(0), x = T(0), y = T(0), z = T(0);
        if (ok) {
            w = ExpOf(-nd * a.inv_radius2);
            x = a.pts[3 * (int64_t)ni + 0];
            y = a.pts[3 * (int64_t)ni + 1];
            z = a.pts[3 * (int64_t)ni + 2];
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
        const int lim = nb.count - base < 64 ? nb.count - base : 64;
        for (int j = 0; j < lim; ++j) {
            const T sw = WaveRead(w, j);
            const T sx = WaveRead(x, j), sy = WaveRead(y, j), sz = WaveRead(z, j);
            if ((m >> j) & 1ull) {
                centroid[0] += sw * sx;
                centroid[1] += sw * sy;
                centroid[2] += sw * sz;
                weight_sum += sw;
            }
        }
    }
    if (weight_sum <= 0) return;
    centroid[0] /= weight_sum;
    centroid[1] /= weight_sum;
    centroid[2] /= weight_sum;

    T covariance[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int base = 0; base < nb.count; base += 64) {
        int ni;
        T nd;
        nb.Load(base, ni, nd);
        const bool ok = ni >= 0;
        T w = T(0), x = T(0), y = T(0), z = T(0);
        if (ok) {
            w = ExpOf(-nd * a.inv_radius2);
            x = a.pts[3 * (int64_t)ni + 0] - centroid[0];
            y = a.pts[3 * (int64_t)ni + 1] - centroid[1];
            z = a.pts[3 * (int64_t)ni + 2] - centroid[2];
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
        const int lim = nb.count - base < 64 ? nb.count - base : 64;
        for (int j = 0; j < lim; ++j) {
            const T sw = WaveRead(w, j);
            const T sx = WaveRead(x, j), sy = WaveRead(y, j), sz = WaveRead(z, j);
            if ((m >> j) & 1ull) {
                covariance[0] += sw * sx * sx;
                covariance[1] += sw * sx * sy;
                covariance[2] += sw * sx * sz;
                covariance[4] += sw * sy * sy;
                covariance[5] += sw * sy * sz;
                covariance[8] += sw * sz * sz;
            }
        }
    }
    covariance[3] = covariance[1];
    covariance[6] = covariance[2];
    covariance[7] = covariance[5];
    if (!writer) return;
    T normal[3];
    // inlined: a call would pass the two arrays through scratch memory
    SmallestEigenvectorSym3Inline<T>(covariance, normal);
    const T projection = (a.pts[po + 0] - centroid[0]) * normal[0] +
                         (a.pts[po + 1] - centroid[1]) * normal[1] +
                         (a.pts[po + 2] - centroid[2]) * normal[2];
    a.out[po + 0] = a.pts[po + 0] - projection * normal[0];
    a.out[po + 1] = a.pts[po + 1] - projection * normal[1];
    a.out[po + 2] = a.pts[po + 2] - projection * normal[2];
    if (a.normals) {
        a.normals[po + 0] = normal[0];
        a.normals[po + 1] = normal[1];
        a.normals[po + 2] = normal[2];
    }
}

// SmoothBilateral's per-point body, PointCloudImpl.h:1700-1751.
template <typename T, typename Nb>
__device__ __forceinline__ void BilateralPoint(const BilateralArgs<T>& a,
                                               int64_t i, const Nb& nb) {
    if (nb.count <= 1) return;
    const int64_t po = 3 * i;
    T nx = a.normals[po + 0];
    T ny = a.normals[po + 1];
    T nz = a.normals[po + 2];
    const T normal_norm = Sqrt(nx * nx + ny * ny + nz * nz);
    if (normal_norm <= 0) return;
    nx /= normal_norm;
    ny /= normal_norm;
    nz /= normal_norm;
    const T qx = a.pts[po + 0], qy = a.pts[po + 1], qz = a.pts[po + 2];
    T weighted_sum[3] = {0, 0, 0};
    T weight_sum = 0;
    for (int base = 0; base < nb.count; base += 64) {
        int ni;
        T nd;
        nb.Load(base, ni, nd);
        const bool ok = ni >= 0;
        T w = T(0), x = T(0), y = T(0), z = T(0);
        if (ok) {
            x = a.pts[3 * (int64_t)ni + 0];
            y = a.pts[3 * (int64_t)ni + 1];
            z = a.pts[3 * (int64_t)ni + 2];
            const T range_distance =
                    (qx - x) * nx + (qy - y) * ny + (qz - z) * nz;
            w = ExpOf(-nd * a.inv_sigma_s2 -
                      range_distance * range_distance * a.inv_sigma_r2);
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
        const int lim = nb.count - base < 64 ? nb.count - base : 64;
        for (int j = 0; j < lim; ++j) {
            const T sw = WaveRead(w, j);
            const T sx = WaveRead(x, j), sy = WaveRead(y, j), sz = WaveRead(z, j);
            if ((m >> j) & 1ull) {
                weighted_sum[0] += sw * sx;
                weighted_sum[1] += sw * sy;
                weighted_sum[2] += sw * sz;
                weight_sum += sw;
            }
        }
    }
    if (weight_sum > 0 && (threadIdx.x & 63) == 0) {
        a.out[po + 0] = weighted_sum[0] / weight_sum;
        a.out[po + 1] = weighted_sum[1] / weight_sum;
        a.out[po + 2] = weighted_sum[2] / weight_sum;
    }
}

// GetCoordinateSystemOnPlane (PointCloudImpl.h:355-380) with the rule its
// comment states: the (0, -nz, ny) branch when |nx| and |ny| are both below
// 1e-6 (the code there tests |nx - nz| and |ny - nz|).
template <typename T>
__device__ __forceinline__ void PlaneFrame(const T* query, T* u, T* v) {
    if (!(Abs(query[0]) < 1e-6) || !(Abs(query[1]) < 1e-6)) {
        const T norm2_inv =
                1.0 / Sqrt(query[0] * query[0] + query[1] * query[1]);
        v[0] = -1 * query[1] * norm2_inv;
        v[1] = query[0] * norm2_inv;
        v[2] = 0;
    } else {
        const T norm2_inv =
                1.0 / Sqrt(query[1] * query[1] + query[2] * query[2]);
        v[0] = 0;
        v[1] = -1 * query[2] * norm2_inv;
        v[2] = query[1] * norm2_inv;
    }
    u[0] = query[1] * v[2] - query[2] * v[1];
    u[1] = query[2] * v[0] - query[0] * v[2];
    u[2] = query[0] * v[1] - query[1] * v[0];
}

// ComputeBoundaryPoints' per-point body, PointCloudImpl.h:471-503: entry 0 of
// the list (the point itself) is skipped; one list of at most 64 entries. The
// angles are sorted by a bitonic network over the wave's lanes (upstream: a
// heap sort in an {N, nn} tensor). A point with a NaN angle is not a boundary
// point.
template <typename T, typename Nb>
__device__ __forceinline__ void BoundaryPoint(const BoundaryArgs<T>& a,
                                              int64_t i, const Nb& nb) {
    if (nb.count - 1 <= 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t po = 3 * i;
    const T normal[3] = {a.normals[po], a.normals[po + 1], a.normals[po + 2]};
    T u[3], v[3];
    PlaneFrame(normal, u, v);
    int ni;
    T nd;
    nb.Load(0, ni, nd);
    const bool active = lane >= 1 && lane < nb.count && ni >= 0;
    T angle = (T)INFINITY;  // sorts after every angle
    if (active) {
        const T delta[3] = {a.pts[3 * (int64_t)ni + 0] - a.pts[po + 0],
                            a.pts[3 * (int64_t)ni + 1] - a.pts[po + 1],
                            a.pts[3 * (int64_t)ni + 2] - a.pts[po + 2]};
        angle = Atan2Of(v[0] * delta[0] + v[1] * delta[1] + v[2] * delta[2],
                        u[0] * delta[0] + u[1] * delta[1] + u[2] * delta[2]);
    }
    if (__builtin_amdgcn_ballot_w64(active && angle != angle) != 0) return;
    const int m = __popcll(__builtin_amdgcn_ballot_w64(active));
    if (m == 0) return;
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const T other = __shfl_xor(angle, j);
            const bool keep_min = ((lane & k) == 0) == ((lane & j) == 0);
            const bool other_less = other < angle;
            angle = (keep_min == other_less) ? other : angle;
        }
    // lanes 0 .. m-1 now hold the angles in ascending order
    const T next = __shfl_down(angle, 1);
    T max_diff = 0;
    if (lane < m - 1) max_diff = next - angle > max_diff ? next - angle : max_diff;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const T o = __shfl_xor(max_diff, s);
        max_diff = max_diff < o ? o : max_diff;
    }
    const T first = __shfl(angle, 0), last = __shfl(angle, m - 1);
    const T diff = 2 * M_PI - last + first;
    max_diff = max_diff < diff ? diff : max_diff;
    if (lane == 0) a.mask[i] = max_diff > a.threshold_rad ? 1 : 0;
}

}  // namespace o3dmi
