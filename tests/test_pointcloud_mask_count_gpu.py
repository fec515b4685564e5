"""GPU tests of the mask-and-count loop the PointCloud operators share
(csrc/pointcloud_rows.h MaskAndCount) and of the count download of their
drivers. Every entry point that returns a mask and a count runs at the sizes
where the tail wave's ballot and the i < n guard can go wrong (1, 63, 64, 65,
257) and, for the four elementwise masks, at 2048 * 256 + 65 rows: the
smallest size at which the capped grid of GridFor(n, 256) takes a second round
whose last wave is partly filled.

The mask buffer holds 0xAB before every call, so a row the loop skips shows.
The mask must equal the numpy oracle's byte for byte and m_out its sum.

Two entries compare a float against a computed threshold (the statistical
filter, the boundary test). Their clouds are built so that no point lies near
the threshold, which the test first proves from the oracle's own float64
numbers; then every mask bit is determined and the comparison is exact."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _pointcloud_filter_oracle as flt
import _pointcloud_sample_oracle as smp
import _pointcloud_smooth_oracle as smo

pytestmark = pytest.mark.gpu

F32, F64 = 0, 1
CODE = {np.float32: F32, np.float64: F64}
POISON = 0xAB

SMALL = (1, 63, 64, 65, 257)
LARGE = 2048 * 256 + 65
# Float64 at n = 65 and at the large size only
ELEMENTWISE = [(n, np.float32) for n in SMALL + (LARGE,)] + \
    [(65, np.float64), (LARGE, np.float64)]
SEARCHING = [(n, np.float32) for n in SMALL] + [(65, np.float64)]


def _L():
    from open3d_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a writable copy


def _vec(v):
    return (C.c_double * len(v))(*[float(x) for x in v])


def _run(name, want, call):
    """call(mask_ptr, m_ref) runs one entry point on a poisoned mask."""
    L = _L()
    n = want.shape[0]
    mask = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
    m = C.c_int64(-1)
    L.check(call(L.ptr(mask), C.byref(m)), name)
    got = mask.cpu().numpy()
    print(name, "n", n, "m_out", m.value, "oracle", int(want.sum()),
          "poison left", int((got == POISON).sum()))
    assert np.array_equal(got, want.astype(np.uint8))
    assert m.value == int(got.sum())


# ---- the elementwise four --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_cloud(n, dtype):
    p = np.random.RandomState(n).uniform(-1, 1, (n, 3)).astype(dtype)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _non_finite_case(n, dtype):
    p = _random_cloud(n, dtype).copy()
    rng = np.random.RandomState(n + 1)
    rows = rng.randint(0, n, max(1, n // 5))
    vals = np.array([np.nan, np.inf, -np.inf], dtype)
    p[rows, rng.randint(0, 3, rows.size)] = vals[rng.randint(0, 3, rows.size)]
    p[n - 1, 2] = np.nan  # the last lane of the tail wave
    want = {(a, b): flt.non_finite_mask(p, a, b)
            for a in (True, False) for b in (True, False)}
    return p, want


@pytest.mark.parametrize("n,dtype", ELEMENTWISE)
def test_remove_non_finite_points(n, dtype):
    p, want = _non_finite_case(n, dtype)
    P = _dev(p)
    lib = _L().lib()
    for (rm_nan, rm_inf), w in want.items():
        _run("remove_non_finite_points", w,
             lambda mask, m: lib.o3dmi_pointcloud_remove_non_finite_points(
                 _L().ptr(P), n, CODE[dtype], int(rm_nan), int(rm_inf), mask, m,
                 None))


@functools.lru_cache(maxsize=None)
def _duplicate_case(n, dtype):
    p = _random_cloud(n, dtype).copy()
    rng = np.random.RandomState(n + 2)
    # a third of the rows repeat an earlier or later row; the last row too
    dst = rng.randint(0, n, n // 3)
    p[dst] = p[rng.randint(0, n, n // 3)]
    p[n - 1] = p[0]
    if n > 2:
        p[1] = 0.0
        p[2] = [0.0, -0.0, 0.0]  # equal numbers, different bits: both kept
    return p, flt.duplicate_mask(p)


@pytest.mark.parametrize("n,dtype", ELEMENTWISE)
def test_remove_duplicated_points(n, dtype):
    p, want = _duplicate_case(n, dtype)
    P = _dev(p)
    lib = _L().lib()
    _run("remove_duplicated_points", want,
         lambda mask, m: lib.o3dmi_pointcloud_remove_duplicated_points(
             _L().ptr(P), n, CODE[dtype], mask, m, None))


LO, HI = (-0.5, -0.25, -1.0), (0.5, 0.75, 0.125)


@functools.lru_cache(maxsize=None)
def _aabb_case(n, dtype):
    p = _random_cloud(n, dtype).copy()
    p[n - 1] = HI  # on the box: both ends are inclusive
    if n > 1:
        p[0] = [LO[0], HI[1], 0.0]
    if n > 2:
        p[1] = [np.nan, 0.0, 0.0]
    return p, smp.aabb_mask(p, LO, HI)


@pytest.mark.parametrize("n,dtype", ELEMENTWISE)
def test_aabb_mask(n, dtype):
    p, want = _aabb_case(n, dtype)
    P = _dev(p)
    lib = _L().lib()
    _run("aabb_mask", want,
         lambda mask, m: lib.o3dmi_pointcloud_aabb_mask(
             _L().ptr(P), n, CODE[dtype], _vec(LO), _vec(HI), mask, m, None))


CENTER, EXTENT = (0.125, -0.25, 0.0), (1.0, 0.5, 1.5)
ROTATION = smo._rotation(np.array([0.3, -0.5, 0.2]))


@functools.lru_cache(maxsize=None)
def _obb_case(n, dtype):
    p = _random_cloud(n, dtype).copy()
    p[n - 1] = CENTER
    if n > 2:
        p[1] = [np.nan, 0.0, 0.0]
    return p, smp.obb_mask(p, CENTER, ROTATION, EXTENT)


@pytest.mark.parametrize("n,dtype", ELEMENTWISE)
def test_obb_mask(n, dtype):
    p, want = _obb_case(n, dtype)
    assert n < 3 or (want.any() and not want.all())
    P = _dev(p)
    lib = _L().lib()
    _run("obb_mask", want,
         lambda mask, m: lib.o3dmi_pointcloud_obb_mask(
             _L().ptr(P), n, CODE[dtype], _vec(CENTER),
             _vec(ROTATION.ravel()), _vec(EXTENT), mask, m, None))


# ---- the four behind a search --------------------------------------------------
RADIUS, NB_POINTS = 0.4, 3


@pytest.mark.parametrize("n,dtype", SEARCHING)
def test_remove_radius_outliers(n, dtype):
    p = _random_cloud(n, dtype)
    want = flt.radius_mask(p, NB_POINTS, RADIUS)
    assert n < 63 or (want.any() and not want.all())
    P = _dev(p)
    lib = _L().lib()
    _run("remove_radius_outliers", want,
         lambda mask, m: lib.o3dmi_pointcloud_remove_radius_outliers(
             _L().ptr(P), n, CODE[dtype], NB_POINTS, C.c_double(RADIUS), mask,
             m, None))


NB_NEIGHBORS, STD_RATIO = 8, 1.0


@pytest.mark.parametrize("n,dtype", SEARCHING)
def test_remove_statistical_outliers(n, dtype):
    p = _random_cloud(n, dtype)
    res = flt.statistical(p, NB_NEIGHBORS, STD_RATIO)
    # no avg_i within 1e-9 of the threshold: the library's float64 tree sums
    # and the oracle's exactly rounded ones give the same mask
    assert flt.guard_band_clear(res) or flt.exactly_degenerate(res)
    assert n < 63 or (res["mask"].any() and not res["mask"].all())
    P = _dev(p)
    lib = _L().lib()
    _run("remove_statistical_outliers", res["mask"],
         lambda mask, m: lib.o3dmi_pointcloud_remove_statistical_outliers(
             _L().ptr(P), n, CODE[dtype], NB_NEIGHBORS, C.c_double(STD_RATIO),
             mask, None, None, m, None))


@pytest.mark.parametrize("n,dtype", SEARCHING)
def test_farthest_point_down_sample(n, dtype):
    p = _random_cloud(n, dtype)
    k, start = (n + 2) // 3, n // 2
    want = smp.farthest_point_mask(p, k, start)
    P = _dev(p)
    lib = _L().lib()
    _run("farthest_point_down_sample", want,
         lambda mask, m: lib.o3dmi_pointcloud_farthest_point_down_sample(
             _L().ptr(P), n, CODE[dtype], k, start, mask, None, m, None))


def _patch(n, dtype):
    """n points: a rows x cols grid of smo.SPACING jittered by 2 % (no two
    angles tie) whose rim is the boundary, and the rest as lone points."""
    rows = int(math.isqrt(n))
    while n % rows and rows * rows + 1 != n:
        rows -= 1
    cols = rows if rows * rows + 1 == n else n // rows
    rng = np.random.RandomState(n)
    x, y = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), np.zeros(rows * cols)], 1) * smo.SPACING
    p[:, :2] += rng.uniform(-0.02, 0.02, (p.shape[0], 2)) * smo.SPACING
    lone = np.array([[5.0 + j, -3.0, 0.0] for j in range(n - rows * cols)])
    p = np.concatenate([p, lone.reshape(-1, 3)])
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    return (np.ascontiguousarray(p.astype(dtype)),
            np.ascontiguousarray(nrm.astype(dtype)))


@pytest.mark.parametrize("n,dtype", SEARCHING)
def test_compute_boundary_points(n, dtype):
    p, nrm = _patch(n, dtype)
    assert p.shape[0] == n
    radius, max_nn = 2.5 * smo.SPACING, 30
    idx, _, counts = smo.hybrid_lists(p, radius, max_nn)
    want, _ = smo.boundary(p, nrm, idx, counts, 90.0, dtype)
    # every largest gap is far from the 90 degree threshold (in float64 too):
    # the rounding of an angle cannot flip a bit
    _, gap64 = smo.boundary(p, nrm, idx, counts, 90.0, np.float64)
    assert (np.abs(gap64 - np.pi / 2) > 1e-2).all()
    assert n < 63 or (want.any() and not want.all())
    P, N = _dev(p), _dev(nrm)
    lib = _L().lib()
    _run("compute_boundary_points", want,
         lambda mask, m: lib.o3dmi_pointcloud_compute_boundary_points(
             _L().ptr(P), _L().ptr(N), n, CODE[dtype], C.c_double(radius),
             max_nn, C.c_double(90.0), mask, m, None))
