"""CPU checks (no GPU) of the host-side proofs behind the frame stream's short
per-voxel update (open3d_amd/csrc/integrate_checks.h), at the edges of their
bounds: the header is compiled on its own with the host C++ compiler."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open3d_amd", "csrc")

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include "integrate_checks.h"
using namespace o3dmi;

static void pose(float e[3][4], float s, float t) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) e[i][j] = (i == j ? s : 0.0f);
    e[0][3] = t;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    float e[3][4];
    // depth scale: RN(1 / s) >= 2^-75 <=> s <= 2^75 (powers of two: exact)
    std::printf("scale_1000 %d\n", SdfDivGuardRedundant(1000.0f, 0.064f));
    std::printf("scale_2p75 %d\n", SdfDivGuardRedundant(0x1p75f, 0.064f));
    std::printf("scale_above_2p75 %d\n",
                SdfDivGuardRedundant(std::nextafter(0x1p75f, inf), 0.064f));
    std::printf("scale_2p76 %d\n", SdfDivGuardRedundant(0x1p76f, 0.064f));
    std::printf("scale_zero %d\n", SdfDivGuardRedundant(0.0f, 0.064f));
    std::printf("scale_inf %d\n", SdfDivGuardRedundant(inf, 0.064f));
    std::printf("scale_nan %d\n", SdfDivGuardRedundant(nan, 0.064f));
    std::printf("trunc_tiny %d\n", SdfDivGuardRedundant(1000.0f, kDivTiny));
    std::printf("trunc_below_tiny %d\n",
                SdfDivGuardRedundant(1000.0f, std::nextafter(kDivTiny, 0.0f)));
    std::printf("trunc_inf %d\n", SdfDivGuardRedundant(1000.0f, inf));
    // pose: per row (2^20 + 1) * res * |voxel| * (|e0| + |e1| + |e2|) + |e3|
    // <= 2^100; with res * voxel = 1 and a diagonal pose the bound on the
    // diagonal entry is 2^100 / (2^20 + 1)
    const double lim = std::ldexp(1.0, 100) / 1048577.0;
    pose(e, 1.0f, 5.0f);
    std::printf("pose_identity %d\n", DepthFoldPoseOk(e, 0.008f, 16, 0.064f));
    pose(e, (float)(lim * 0.999), 0.0f);
    std::printf("pose_below_edge %d\n", DepthFoldPoseOk(e, 0.5f, 2, 0.064f));
    pose(e, (float)(lim * 1.001), 0.0f);
    std::printf("pose_above_edge %d\n", DepthFoldPoseOk(e, 0.5f, 2, 0.064f));
    pose(e, 1.0f, 0x1p99f);
    std::printf("pose_translation_2p99 %d\n",
                DepthFoldPoseOk(e, 0.008f, 16, 0.064f));
    pose(e, 1.0f, 0x1p101f);
    std::printf("pose_translation_2p101 %d\n",
                DepthFoldPoseOk(e, 0.008f, 16, 0.064f));
    pose(e, 1.0f, 0.0f);
    e[2][1] = inf;
    std::printf("pose_inf %d\n", DepthFoldPoseOk(e, 0.008f, 16, 0.064f));
    pose(e, 1.0f, 0.0f);
    e[1][3] = nan;
    std::printf("pose_nan %d\n", DepthFoldPoseOk(e, 0.008f, 16, 0.064f));
    pose(e, 1.0f, 0.0f);
    std::printf("voxel_inf %d\n", DepthFoldPoseOk(e, inf, 16, 0.064f));
    std::printf("fold_trunc_inf %d\n", DepthFoldPoseOk(e, 0.008f, 16, inf));
    std::printf("fold_trunc_nan %d\n", DepthFoldPoseOk(e, 0.008f, 16, nan));
    return 0;
}
"""

WANT = {
    "scale_1000": 1, "scale_2p75": 1, "scale_above_2p75": 0, "scale_2p76": 0,
    "scale_zero": 0, "scale_inf": 0, "scale_nan": 0, "trunc_tiny": 1,
    "trunc_below_tiny": 0, "trunc_inf": 0,
    "pose_identity": 1, "pose_below_edge": 1, "pose_above_edge": 0,
    "pose_translation_2p99": 1, "pose_translation_2p101": 0, "pose_inf": 0,
    "pose_nan": 0, "voxel_inf": 0, "fold_trunc_inf": 0, "fold_trunc_nan": 0,
}


def test_host_checks_at_their_edges(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "checks.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "checks"
    # the product's host flags that matter here: no contraction, IEEE floats
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off",
                           "-I" + CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True,
                         check=True).stdout
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
    assert got == WANT
