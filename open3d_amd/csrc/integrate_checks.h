// Host-side proofs behind the frame-step kernel's short per-voxel update
// (IntegrateRoleWide's apply in vbg_stream.hip). Each holds for a whole launch;
// a launch that fails one takes the IEEE-division form of the kernel, which
// keeps every per-voxel test (same results, see vbg_stream.hip). Plain C++ with
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

}  // namespace o3dmi
