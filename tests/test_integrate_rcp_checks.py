"""CPU checks (no GPU) of RcpRangePoseOk (open3d_amd/csrc/integrate_checks.h),
the host-side proof that lets the frame stream's integrate role drop the range
test of the projection's 1 / z: the header is compiled on its own with the host
C++ compiler, asked about poses at the edges of its bounds, and used as the
filter of a float32 search for a counter-example to what it promises -- no
voxel of an accepted pose has 0 < z < 2^-60."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open3d_amd", "csrc")

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "integrate_checks.h"
using namespace o3dmi;

static void pose(float e[3][4], float s, float t) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) e[i][j] = (i == j ? s : 0.0f);
    e[2][3] = t;
}

// filter mode: records of 14 floats (e row-major, voxel size, resolution) ->
// one byte per record
static int filter(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    FILE* o = std::fopen(out, "wb");
    if (!f || !o) return 1;
    float r[14];
    while (std::fread(r, sizeof(float), 14, f) == 14) {
        float e[3][4];
        for (int i = 0; i < 12; ++i) e[i / 4][i % 4] = r[i];
        std::fputc(RcpRangePoseOk(e, r[12], (int)r[13]) ? 1 : 0, o);
    }
    std::fclose(f);
    return std::fclose(o);
}

int main(int argc, char** argv) {
    if (argc == 3) return filter(argv[1], argv[2]);
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    float e[3][4];
    const float ts[] = {0.0f, -0.0f, 0x1p-37f, -0x1p-37f, 0x1p-36f, -0x1p-36f,
                        std::nextafter(0x1p-36f, 0.0f), nan, inf, -inf, 0.44f};
    const char* names[] = {"t_zero", "t_neg_zero", "t_2m37", "t_neg_2m37",
                           "t_2m36", "t_neg_2m36", "t_below_2m36", "t_nan",
                           "t_inf", "t_neg_inf", "t_ordinary"};
    for (int k = 0; k < 11; ++k) {
        pose(e, 1.0f, ts[k]);
        std::printf("%s %d\n", names[k], RcpRangePoseOk(e, 0.008f, 16));
    }
    // third row: (2^20 + 1) * res * |voxel| * (|e20| + |e21| + |e22|) + |e23|
    // <= 2^59; with res * voxel = 1 and a diagonal pose the bound on e22 is
    // (2^59 - |e23|) / (2^20 + 1)
    const double lim = std::ldexp(1.0, 59) / 1048577.0;
    pose(e, (float)(lim * 0.999), 1.0f);
    std::printf("row_below_edge %d\n", RcpRangePoseOk(e, 0.5f, 2));
    pose(e, (float)(lim * 1.001), 1.0f);
    std::printf("row_above_edge %d\n", RcpRangePoseOk(e, 0.5f, 2));
    pose(e, 1.0f, 0x1p58f);
    std::printf("t_2p58 %d\n", RcpRangePoseOk(e, 0.008f, 16));
    pose(e, 1.0f, 0x1p60f);
    std::printf("t_2p60 %d\n", RcpRangePoseOk(e, 0.008f, 16));
    // only the third row counts
    pose(e, 1.0f, 0.44f);
    e[0][3] = 0x1p90f;
    std::printf("other_rows_large %d\n", RcpRangePoseOk(e, 0.008f, 16));
    pose(e, 1.0f, 0.44f);
    e[2][0] = nan;
    std::printf("row_nan %d\n", RcpRangePoseOk(e, 0.008f, 16));
    pose(e, 1.0f, 0.44f);
    e[2][1] = inf;
    std::printf("row_inf %d\n", RcpRangePoseOk(e, 0.008f, 16));
    pose(e, 1.0f, 0.44f);
    std::printf("voxel_inf %d\n", RcpRangePoseOk(e, inf, 16));
    std::printf("voxel_nan %d\n", RcpRangePoseOk(e, nan, 16));
    std::printf("res_zero %d\n", RcpRangePoseOk(e, 0.008f, 0));
    return 0;
}
"""

WANT = {
    "t_zero": 0, "t_neg_zero": 0, "t_2m37": 0, "t_neg_2m37": 0, "t_2m36": 1,
    "t_neg_2m36": 1, "t_below_2m36": 0, "t_nan": 0, "t_inf": 0,
    "t_neg_inf": 0, "t_ordinary": 1,
    "row_below_edge": 1, "row_above_edge": 0, "t_2p58": 1, "t_2p60": 0,
    "other_rows_large": 1, "row_nan": 0, "row_inf": 0, "voxel_inf": 0,
    "voxel_nan": 0, "res_zero": 0,
}


@pytest.fixture(scope="module")
def checks_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("rcp_checks")
    src = d / "checks.cpp"
    src.write_text(DRIVER)
    exe = d / "checks"
    # the product's host flags that matter here: no contraction, IEEE floats
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off",
                           "-I" + CSRC, str(src), "-o", str(exe)])
    return str(exe), d


def test_rcp_range_check_at_its_edges(checks_exe):
    exe, _ = checks_exe
    out = subprocess.run([exe], capture_output=True, text=True,
                         check=True).stdout
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
    assert got == WANT


# ---- the search -------------------------------------------------------------
# The kernel's z (IntegrateRoleWide's issue block, Camera::RigidTransform's
# order): the voxel coordinates times the voxel size, then
# ((x e20 + y e21) + z e22) + e23, every operation rounded to float32.
RES = 16
KEY_RANGE = (1 << 20) * RES  # |voxel coordinate| over every block key
F = np.float32
TINY = F(2.0 ** -60)


def _kernel_z(e2, voxel, xyz):
    xs, ys, zs = (xyz[:, i].astype(F) * voxel for i in range(3))
    a = (xs * e2[:, 0] + ys * e2[:, 1]) + zs * e2[:, 2]
    return a, a + e2[:, 3]


def _adversarial(rng, n, row_exp):
    """Third rows, voxel sizes and voxel coordinates with the translation set
    next to the value that cancels the sum of the products: e23 = -a moved by
    -3 .. 3 float32 steps, the only place a tiny z can come from."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    scale = 2.0 ** rng.uniform(row_exp[0], row_exp[1], size=(n, 1))
    e2 = np.zeros((n, 4), F)
    e2[:, :3] = (d * scale).astype(F)
    voxel = rng.choice(np.array([0.004, 0.008, 0.05, 1.0], F), size=n)
    mag = np.floor(2.0 ** rng.uniform(0, np.log2(KEY_RANGE), size=(n, 3)))
    xyz = (mag * rng.choice([-1, 1], size=(n, 3))).astype(np.int64)
    a, _ = _kernel_z(e2, voxel, xyz)
    t = -a
    for _ in range(3):  # up to 3 steps away, either side
        step = rng.integers(-1, 2, size=n)
        t = np.where(step > 0, np.nextafter(t, F(np.inf)),
                     np.where(step < 0, np.nextafter(t, F(-np.inf)), t))
    e2[:, 3] = t.astype(F)
    return e2, voxel, xyz


def _accepted(checks_exe, e2, voxel):
    exe, d = checks_exe
    n = len(e2)
    rec = np.zeros((n, 14), F)
    rec[:, 0] = rec[:, 5] = 1.0  # rows 0 and 1: any finite values
    rec[:, 8:12] = e2
    rec[:, 12] = voxel
    rec[:, 13] = RES
    fin, fout = str(d / "poses.bin"), str(d / "accept.bin")
    rec.tofile(fin)
    subprocess.check_call([exe, fin, fout])
    ok = np.fromfile(fout, np.uint8)
    assert len(ok) == n
    return ok.astype(bool)


def test_no_accepted_pose_gives_a_tiny_positive_z(checks_exe):
    rng = np.random.default_rng(9)
    seen_small_row = 0
    # rows from far below the translation bound (|a| around 2^-36 and less)
    # to ordinary rotations and beyond
    for row_exp in ((-62, -30), (-30, 0), (0, 12)):
        e2, voxel, xyz = _adversarial(rng, 200000, row_exp)
        ok = _accepted(checks_exe, e2, voxel)
        assert ok.any()
        _, z = _kernel_z(e2[ok], voxel[ok], xyz[ok])
        bad = (z > 0) & (z < TINY)
        assert not bad.any(), (e2[ok][bad][:3], z[bad][:3])
        # the cancellation is really there: z = 0 and z of a few steps occur
        assert (z == 0).any() and ((z > 0) & (z < F(1e-3))).any()
        seen_small_row += int(ok.sum())
    assert seen_small_row > 100000


def test_the_search_finds_tiny_z_for_rejected_poses(checks_exe):
    """The same search has teeth: with translations below 2^-36 (which the
    check rejects) it does come across 0 < z < 2^-60."""
    rng = np.random.default_rng(10)
    e2, voxel, xyz = _adversarial(rng, 200000, (-62, -38))
    ok = _accepted(checks_exe, e2, voxel)
    small_t = np.abs(e2[:, 3]) < F(2.0 ** -36)
    assert not (ok & small_t).any()
    _, z = _kernel_z(e2[~ok], voxel[~ok], xyz[~ok])
    assert ((z > 0) & (z < TINY)).any()
