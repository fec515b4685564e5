"""CPU checks of the sampling / cropping oracle
(tests/_pointcloud_sample_oracle.py) against the golden vectors, of the
library's pure permutation o3dmi_sample_index against the oracle's, and of
every argument error the new calls answer before their first launch. No GPU."""
import ctypes as C

import numpy as np
import pytest

import _pointcloud_sample_oracle as orc

INVALID_ARG, UNSUPPORTED = 1, 7
F32, F64, I32 = 0, 1, 4
DTYPES = [np.float32, np.float64]
FAKE = C.c_void_p(0x1000)  # never dereferenced: the checks come first


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from open3d_amd import _lib
    return _lib.lib()


# ---- the oracle against the golden vectors -----------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_farthest_point_oracle_matches_goldens(dtype):
    cases = orc.reference_vectors()["farthest_point"]
    assert [c["name"] for c in cases] == ["upstream_start0", "upstream_start4",
                                          "duplicates"]
    for case in cases:
        pts = np.array(case["points"], dtype)
        order = orc.farthest_point_order(pts, case["num_samples"],
                                         case["start_index"])
        assert sorted(set(order.tolist())) == case["expected_indices"], case
        if "expected_order" in case:
            assert order.tolist() == case["expected_order"]
        mask = orc.farthest_point_mask(pts, case["num_samples"],
                                       case["start_index"])
        assert np.flatnonzero(mask).tolist() == case["expected_indices"]


def test_farthest_point_golden_pins_the_lowest_index():
    """After samples 0 and 5 of upstream's case, 3 and 6 tie for the next."""
    pts = np.array(orc.reference_vectors()["farthest_point"][0]["points"],
                   np.float32)
    d = np.minimum(((pts - pts[0]) ** 2).sum(axis=1),
                   ((pts - pts[5]) ** 2).sum(axis=1))
    assert d[3] == d[6] == d.max() and (d == d.max()).sum() == 2
    assert orc.farthest_point_order(pts, 3, 0).tolist() == [0, 5, 3]


def test_duplicates_give_fewer_rows_than_samples():
    case = orc.reference_vectors()["farthest_point"][2]
    mask = orc.farthest_point_mask(np.array(case["points"]), 4, 0)
    assert mask.sum() == 2


def test_uniform_golden():
    v = orc.reference_vectors()["uniform"]
    pts = np.array(v["points"], np.float32)
    rows = list(range(0, len(pts), v["every_k_points"]))
    assert rows == v["expected_rows"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_crop_oracle_matches_goldens(dtype):
    v = orc.reference_vectors()
    for case in v["aabb"]:
        m = orc.aabb_mask(np.array(case["points"], dtype), case["min_bound"],
                          case["max_bound"])
        assert np.flatnonzero(m).tolist() == case["expected_indices"]
    assert len(v["obb"]) == 2
    for case in v["obb"]:
        m = orc.obb_mask(np.array(case["points"], dtype), case["center"],
                         case["rotation"], case["extent"])
        assert np.flatnonzero(m).tolist() == case["expected_indices"], case


# ---- the permutation -----------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 1000, 4097])
def test_sample_index_is_a_bijection_and_equals_the_oracle(lib, n):
    for seed in (0, 0xDEADBEEFCAFEF00D):
        got = [lib.o3dmi_sample_index(seed, n, j) for j in range(n)]
        assert sorted(got) == list(range(n))
        assert got == [orc.sample_index(seed, n, j) for j in range(n)]


def test_sample_index_depends_on_the_seed_and_refuses_bad_entries(lib):
    n, m = 1000, 100
    a = [lib.o3dmi_sample_index(1, n, j) for j in range(m)]
    b = [lib.o3dmi_sample_index(2, n, j) for j in range(m)]
    assert a != b
    assert a != list(range(m))
    assert lib.o3dmi_sample_index(0, 10, -1) == -1
    assert lib.o3dmi_sample_index(0, 10, 10) == -1
    assert lib.o3dmi_sample_index(0, 0, 0) == -1
    assert lib.o3dmi_sample_index(0, 1 << 62, 0) == -1


def test_farthest_point_capacity_is_reported(lib):
    c32 = lib.o3dmi_pointcloud_farthest_point_capacity(F32)
    c64 = lib.o3dmi_pointcloud_farthest_point_capacity(F64)
    assert c32 > c64 >= 1024
    assert lib.o3dmi_pointcloud_farthest_point_capacity(I32) == 0


# ---- argument errors, all before the first launch ------------------------------
def test_farthest_point_argument_errors(lib):
    order = lib.o3dmi_pointcloud_farthest_point_order
    down = lib.o3dmi_pointcloud_farthest_point_down_sample
    m = C.c_int64(-5)

    def both(n, dtype, k, start, points=FAKE):
        a = order(points, n, dtype, k, start, 0, FAKE, None)
        b = down(points, n, dtype, k, start, FAKE, None, C.byref(m), None)
        assert a == b
        return a

    assert both(10, F32, 11, 0) == INVALID_ARG       # more samples than points
    assert both(10, F32, 4, 10) == INVALID_ARG       # start outside [0, n)
    assert both(10, F32, 4, -1) == INVALID_ARG
    assert both(-1, F32, 0, 0) == INVALID_ARG
    assert both(10, I32, 4, 0) == INVALID_ARG        # dtype
    assert both(10, F64, 4, 0, points=None) == INVALID_ARG
    assert both(1 << 27, F32, 4, 0) == INVALID_ARG   # n out of range
    assert both(10, F32, -1, 0) == INVALID_ARG
    assert m.value == -5                             # outputs untouched
    assert order(FAKE, 10, F32, 4, 0, 3, FAKE, None) == INVALID_ARG  # form
    assert order(FAKE, 10, F32, 4, 0, 0, None, None) == INVALID_ARG
    assert down(FAKE, 10, F32, 4, 0, None, None, C.byref(m), None) \
        == INVALID_ARG
    assert down(FAKE, 10, F32, 4, 0, FAKE, None, None, None) == INVALID_ARG
    # the resident form above its capacity: unsupported, not invalid
    for dtype in (F32, F64):
        cap = lib.o3dmi_pointcloud_farthest_point_capacity(dtype)
        assert order(FAKE, cap + 1, dtype, 4, 0, 1, FAKE, None) == UNSUPPORTED
    # an empty cloud with no samples is fine
    assert both(0, F32, 0, 0, points=None) == 0
    assert m.value == 0


def test_uniform_and_random_argument_errors(lib):
    uni = lib.o3dmi_pointcloud_uniform_down_sample
    m = C.c_int64(-5)
    ins = (C.c_void_p * 1)(0x1000)
    outs = (C.c_void_p * 1)(0x2000)
    widths = (C.c_int64 * 1)(12)
    for k in (0, -3):
        assert uni(8, k, 1, ins, widths, outs, C.byref(m), None) == INVALID_ARG
    assert uni(-1, 1, 1, ins, widths, outs, C.byref(m), None) == INVALID_ARG
    assert uni(8, 1, 0, ins, widths, outs, C.byref(m), None) == INVALID_ARG
    assert uni(8, 1, 9, ins, widths, outs, C.byref(m), None) == INVALID_ARG
    assert uni(8, 1, 1, ins, widths, outs, None, None) == INVALID_ARG
    assert m.value == -5
    assert uni(0, 3, 1, ins, widths, outs, C.byref(m), None) == 0
    assert m.value == 0

    rnd = lib.o3dmi_pointcloud_random_sample_indices
    m = C.c_int64(-5)
    for ratio in (-0.1, 1.5, float("nan"), float("inf")):
        assert rnd(100, ratio, 0, FAKE, C.byref(m), None) == INVALID_ARG
    assert rnd(-1, 0.5, 0, FAKE, C.byref(m), None) == INVALID_ARG
    assert rnd(100, 0.5, 0, None, C.byref(m), None) == INVALID_ARG
    assert rnd(100, 0.5, 0, FAKE, None, None) == INVALID_ARG
    assert m.value == -5
    assert rnd(100, 0.0, 0, None, C.byref(m), None) == 0 and m.value == 0
    assert rnd(1, 0.5, 0, None, C.byref(m), None) == 0 and m.value == 0


def test_crop_and_bound_argument_errors(lib):
    aabb = lib.o3dmi_pointcloud_aabb_mask
    obb = lib.o3dmi_pointcloud_obb_mask
    m = C.c_int64(-5)
    v = lambda *x: (C.c_double * len(x))(*x)
    eye = v(1, 0, 0, 0, 1, 0, 0, 0, 1)
    assert aabb(FAKE, 4, F32, v(0, 0, 0), v(1, -1, 1), FAKE, C.byref(m),
                None) == INVALID_ARG                 # max < min on one axis
    assert aabb(FAKE, 4, F32, v(0, 0, 0), v(1, float("nan"), 1), FAKE,
                C.byref(m), None) == INVALID_ARG
    assert aabb(FAKE, 4, I32, v(0, 0, 0), v(1, 1, 1), FAKE, C.byref(m),
                None) == INVALID_ARG
    assert aabb(None, 4, F32, v(0, 0, 0), v(1, 1, 1), FAKE, C.byref(m),
                None) == INVALID_ARG
    assert aabb(FAKE, 4, F32, None, v(1, 1, 1), FAKE, C.byref(m),
                None) == INVALID_ARG
    assert aabb(FAKE, 4, F32, v(0, 0, 0), v(1, 1, 1), FAKE, None,
                None) == INVALID_ARG
    assert obb(FAKE, 4, F64, v(0, 0, 0), eye, v(1, -1, 1), FAKE, C.byref(m),
               None) == INVALID_ARG                  # negative extent
    assert obb(FAKE, -1, F64, v(0, 0, 0), eye, v(1, 1, 1), FAKE, C.byref(m),
               None) == INVALID_ARG
    assert obb(FAKE, 4, F64, v(0, 0, 0), None, v(1, 1, 1), FAKE, C.byref(m),
               None) == INVALID_ARG
    assert m.value == -5
    # an empty box is no error at the ABI; neither is an empty cloud
    assert aabb(None, 0, F32, v(0, 0, 0), v(0, 1, 1), None, C.byref(m),
                None) == 0 and m.value == 0

    bound = lib.o3dmi_pointcloud_min_max_bound
    lo, hi = v(7, 7, 7), v(7, 7, 7)
    assert bound(FAKE, -1, F32, lo, hi, None) == INVALID_ARG
    assert bound(FAKE, 4, I32, lo, hi, None) == INVALID_ARG
    assert bound(None, 4, F32, lo, hi, None) == INVALID_ARG
    assert bound(FAKE, 4, F32, None, hi, None) == INVALID_ARG
    assert list(lo) == [7, 7, 7]
    assert bound(None, 0, F32, lo, hi, None) == 0    # zeros, as upstream
    assert list(lo) == [0, 0, 0] and list(hi) == [0, 0, 0]
