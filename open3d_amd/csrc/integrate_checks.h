// Host-side proofs behind the frame-step kernel's short per-voxel update
// (IntegrateRoleWide's apply in vbg_stream.hip). Each holds for a whole launch;
// a launch that fails one takes the IEEE-division form of the kernel, which
// keeps every per-voxel test (same results, see vbg_stream.hip); a launch that
// passes those but fails RcpRangePoseOk keeps the short update with the range
// test of the projection's reciprocal. Plain C++ with
// no HIP dependency, so that tests/test_integrate_host_checks.py can compile
// it on its own.
#pragma once

#include <cmath>

namespace o3dmi {

// Lower bound of the magnitudes DivByConst handles itself; smaller inputs
// (zeros, denormals and their neighbourhood, where the exact-residual argument
// needs gradual underflow to cooperate) take the IEEE sequence.
constexpr float kDivTiny = 1.0e-30f;

// |voxel coordinate| / resolution over every block key (21-bit block
// coordinates with bias 2^20, common.h kKeyBias): below 2^20 + 1.
constexpr double kFoldCoordPerRes = 1048577.0;
// Bound kept on every row of the rigid transform: far below FLT_MAX (2^128),
// so the handful of float roundings on the way (each <= 1 + 2^-24) cannot
// overflow.
constexpr double kFoldTransformBound = 0x1p100;

// Invalid depths as -inf in the prepared records (item "depth fold" in
// vbg_stream.hip): apply may then drop its two depth tests, because
// -inf - z < -sdf_trunc for every z that is not NaN and every finite
// sdf_trunc. z is the third row of the voxel's rigid transform: it is finite
// when the extrinsic and the voxel size are finite and no row can overflow.
// `e` is the float extrinsic the kernel uses (Camera::Make of the host 4x4).
inline bool DepthFoldPoseOk(const float e[3][4], float voxel_size,
                            int resolution, float sdf_trunc) {
    if (!std::isfinite(voxel_size) || !std::isfinite(sdf_trunc) ||
        resolution <= 0)
        return false;
    const double c = kFoldCoordPerRes * (double)resolution *
                     std::fabs((double)voxel_size);
    for (int i = 0; i < 3; ++i) {
        double s = 0.0;
        for (int j = 0; j < 4; ++j) {
            if (!std::isfinite(e[i][j])) return false;
            s += std::fabs((double)e[i][j]) * (j < 3 ? c : 1.0);
        }
        if (!(s <= kFoldTransformBound)) return false;
    }
    return true;
}

// The underflow guard of sdf / sdf_trunc (|cl| < kDivTiny -> IEEE division)
// is unreachable when every valid depth is at least 2^-75 and the truncation
// distance at least kDivTiny. cl = min(d - z, sdf_trunc) with d a valid depth,
// d >= RN(1 / depth_scale) (the smallest non-zero uint16 depth over the scale,
// correctly rounded; the division is monotone). If |d - z| < 1e-30 then z lies
// in [d / 2, 2 d] (d >= 2^-75), so d - z is exact (Sterbenz) and, both being
// multiples of 2^-99 (floats >= 2^-76), either +0 or at least 2^-99 > 1e-30
// in magnitude. cl = sdf_trunc >= kDivTiny otherwise. DivByConst(+0) = +0,
// the IEEE quotient; every other cl is in the range VerifyFastDivision proved.
inline bool SdfDivGuardRedundant(float depth_scale, float sdf_trunc) {
    if (!(depth_scale > 0.0f) || !std::isfinite(depth_scale)) return false;
    const float min_depth = 1.0f / depth_scale;  // RN(1 / depth_scale)
    return min_depth >= 0x1p-75f && sdf_trunc >= kDivTiny &&
           std::isfinite(sdf_trunc);
}

// Bound kept on the third row of the rigid transform by RcpRangePoseOk: with
// the float roundings on the way (three adds and four products, each
// <= 1 + 2^-24) z stays below 2^60, the upper end of the verified range of
// the projection's short reciprocal.
constexpr double kRcpRowBound = 0x1p59;
// Smallest |e[2][3]| RcpRangePoseOk accepts.
constexpr float kRcpMinTranslation = 0x1p-36f;

// The range test of the projection's 1 / z (RcpOutOfRange in vbg_stream.hip:
// the short reciprocal is verified for [2^-60, 2^60], every other z takes the
// IEEE division) is redundant for a launch whose poses pass this check. A
// voxel with z <= 0 (or a NaN, which DepthFoldPoseOk excludes) is rejected by
// the update whatever its projection was, and its gather address is made safe
// by the in-image select, so only 0 < z outside the range matters.
//   Upper end: |z| <= (|e20| + |e21| + |e22|) c + |e23| <= 2^59 in exact
// arithmetic, c as in DepthFoldPoseOk; the roundings keep it below 2^60.
//   Lower end: z leaves the transform as RN(a + t), t = e[2][3] and a the
// float32 sum of the three products (((x e20) + y e21) + z e22: the kernel
// adds the translation last). Suppose |t| >= 2^-36, z != 0 and |z| < 2^-60.
// 2^-60 is a float and rounding is monotone, so |a + t| < 2^-60 and
// |a| > |t| - 2^-60 >= 2^-37. A float of magnitude >= 2^-37 is a multiple of
// 2^-60 (its ulp is at least 2^-37-23), so a + t is a multiple of 2^-60 of
// magnitude below 2^-60: a + t = 0 and z = 0, a contradiction. Hence z is
// zero, negative or at least 2^-60.
// A pose with a smaller |e[2][3]| (the identity: the first frame of most runs)
// fails the check and its launch keeps the range test.
inline bool RcpRangePoseOk(const float e[3][4], float voxel_size,
                           int resolution) {
    if (!std::isfinite(voxel_size) || resolution <= 0) return false;
    const double c = kFoldCoordPerRes * (double)resolution *
                     std::fabs((double)voxel_size);
    double s = 0.0;
    for (int j = 0; j < 4; ++j) {
        if (!std::isfinite(e[2][j])) return false;
        s += std::fabs((double)e[2][j]) * (j < 3 ? c : 1.0);
    }
    return s <= kRcpRowBound && std::fabs(e[2][3]) >= kRcpMinTranslation;
}

}  // namespace o3dmi
