// Symmetric 3x3 eigen-decomposition shared by the normal estimation
// (normals.hip), the colour-gradient solve, the MLS projection
// (pointcloud_smooth_device.h) and, on the host, the frames of the bounding
// volumes (host/bounding_volume.cpp): the Jacobi iteration compiles for both
// sides, everything below it is device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace o3dmi {

__host__ __device__ __forceinline__ float Sqrt(float v) { return sqrtf(v); }
__host__ __device__ __forceinline__ double Sqrt(double v) { return sqrt(v); }
__host__ __device__ __forceinline__ float Abs(float v) { return fabsf(v); }
__host__ __device__ __forceinline__ double Abs(double v) { return fabs(v); }

// ---- symmetric 3x3 eigen-decomposition (this code base's own) -----------------
// Cyclic Jacobi: rotations in the (0,1), (0,2), (1,2) planes, each chosen to
// annihilate that off-diagonal entry (the smaller root of t^2 + 2 theta t - 1),
// until every off-diagonal entry is an exact zero or kJacobiSweeps sweeps have
// run (quadratic convergence: a 3x3 is at rounding level after 4 - 5). On
// return a is diagonal (eigenvalues, unsorted) and the columns of V are the
// eigenvectors. Used by the normal estimation (smallest eigenvector) and by
// the colour-gradient solve (pseudo-inverse).
constexpr int kJacobiSweeps = 8;
template <typename T>
__host__ __device__ __forceinline__ void JacobiEigenSym3(T (&a)[3][3],
                                                         T (&V)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? T(1) : T(0);
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const T apq = a[p][q];
                if (apq == T(0)) continue;
                const T theta = (a[q][q] - a[p][p]) / (T(2) * apq);
                const T t = (theta >= T(0) ? T(1) : T(-1)) /
                            (Abs(theta) + Sqrt(theta * theta + T(1)));
                const T c = T(1) / Sqrt(t * t + T(1));
                const T sn = t * c;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const T akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - sn * akq;
                    a[k][q] = sn * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const T apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - sn * aqk;
                    a[q][k] = sn * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const T vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - sn * vkq;
                    V[k][q] = sn * vkp + c * vkq;
                }
            }
    }
}

// Normal of a neighbourhood = unit eigenvector of the smallest eigenvalue of
// its covariance. The reference (EstimatePointWiseNormalsWithFastEigen3x3,
// t/geometry/kernel/PointCloudImpl.h:875-1009) gets it non-iteratively in the
// point dtype (trigonometric eigenvalues + cross products of rows); this
// routine is NOT that one: the covariance is widened to float64 and diagonalised
// by the converged Jacobi above, so the answer is the exact eigenvector to
// float64 rounding for both dtypes. Against the reference's compiled body the
// two agree to the reference's own rounding: <= 1e-4 rad (Float32) / 1e-10
// (Float64) wherever the two smallest eigenvalues are separated by more than
// 5 % of the largest (tests/test_normals_gpu.py); in a degenerate eigenspace
// any of its unit vectors is a valid answer and the two routines pick
// different ones.
//   * sign: an eigenvector has none, the reference's is whatever its cross
//     products produce. Pinned here: the last non-zero component is positive
//     (z > 0, else y > 0, else x > 0) -- the convention the reference's own
//     value test satisfies (cpp/tests/t/geometry/PointCloud.cpp:630-668);
//   * ties between eigenvalues go to the later axis, so the identity
//     covariance of a neighbourhood with < 3 members gives +z as in the
//     reference; an all-zero covariance has no direction: zero vector (the
//     caller turns it into +z when the cloud has no prior normals).
template <typename T>
__device__ __forceinline__ void SmallestEigenvectorSym3Inline(const T* cov,
                                                               T* nrm) {
    double a[3][3], V[3][3];
    double scale = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double m = fabs((double)cov[i]);
        scale = m > scale ? m : scale;
    }
    if (!(scale > 0.0)) {
        nrm[0] = nrm[1] = nrm[2] = T(0);
        return;
    }
    // symmetric by construction: the upper triangle is read
    const double inv = 1.0 / scale;
    a[0][0] = (double)cov[0] * inv;
    a[1][1] = (double)cov[4] * inv;
    a[2][2] = (double)cov[8] * inv;
    a[0][1] = a[1][0] = (double)cov[1] * inv;
    a[0][2] = a[2][0] = (double)cov[2] * inv;
    a[1][2] = a[2][1] = (double)cov[5] * inv;
    JacobiEigenSym3<double>(a, V);
    int best = 0;
    if (a[1][1] <= a[best][best]) best = 1;
    if (a[2][2] <= a[best][best]) best = 2;
    double v[3] = {V[0][best], V[1][best], V[2][best]};
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const bool flip = v[2] < 0.0 ||
                      (v[2] == 0.0 && (v[1] < 0.0 || (v[1] == 0.0 && v[0] < 0.0)));
    const double s = (flip ? -1.0 : 1.0) / len;
    nrm[0] = (T)(v[0] * s);
    nrm[1] = (T)(v[1] * s);
    nrm[2] = (T)(v[2] * s);
}

// The same as a function of its own, for callers with registers to spare for
// a call (normals.hip).
template <typename T>
__device__ void SmallestEigenvectorSym3(const T* cov, T* nrm) {
    SmallestEigenvectorSym3Inline<T>(cov, nrm);
}

}  // namespace o3dmi
