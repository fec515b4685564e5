"""CPU checks (no GPU) of the PointCloud selection / filter family: the numpy
oracle against the reference's own unit-test vectors, the new symbols in the
header and the library, the host guards, and the guard band that makes the
statistical mask of the GPU tests well defined."""
import ctypes as C
import os

import numpy as np
import pytest

import _pointcloud_filter_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 7

NAMES = ("o3dmi_pointcloud_select_by_mask",
         "o3dmi_pointcloud_select_by_index",
         "o3dmi_pointcloud_remove_non_finite_points",
         "o3dmi_pointcloud_remove_duplicated_points",
         "o3dmi_pointcloud_remove_radius_outliers",
         "o3dmi_pointcloud_remove_statistical_outliers",
         "o3dmi_slac_preprocess_point_cloud")


# ---- 1. the oracle against the reference's vectors ----------------------------
def test_oracle_select_by_mask_reference_vector():
    v = orc.reference_vectors()["select"]
    pts = orc.f32(v["points"])
    m = v["by_mask"]
    got = orc.select_by_mask({"positions": pts}, m["mask"])["positions"]
    assert np.array_equal(got, orc.f32(m["expected"]))
    got = orc.select_by_mask({"positions": pts}, m["mask"], True)["positions"]
    assert np.array_equal(got, orc.f32(m["expected_inverted"]))


def test_oracle_select_by_index_reference_vectors():
    v = orc.reference_vectors()["select"]
    pts = orc.f32(v["points"])
    assert len(v["by_index"]) == 6
    for case in v["by_index"]:
        got = orc.select_by_index({"positions": pts}, case["indices"],
                                  pts.shape[0], case["invert"],
                                  case["remove_duplicates"])["positions"]
        assert np.array_equal(got, orc.f32(case["expected"])), case


def test_oracle_radius_outliers_reference_vector():
    v = orc.reference_vectors()["radius_outliers"]
    pts = orc.f32(v["points"])
    mask = orc.radius_mask(pts, v["nb_points"], v["search_radius"])
    assert np.array_equal(pts[mask], orc.f32(v["expected"]))


def test_oracle_duplicated_points_reference_vector():
    v = orc.reference_vectors()["duplicated_points"]
    pts = orc.f32(v["points"])
    mask = orc.duplicate_mask(pts)
    assert np.array_equal(pts[mask], orc.f32(v["expected"]))
    assert mask.tolist() == [True, False, True, False, True, True]


def test_oracle_non_finite_points_reference_vectors():
    v = orc.reference_vectors()["non_finite_points"]
    pts = orc.f32(v["points"])
    assert len(v["forms"]) == 4
    for form in v["forms"]:
        mask = orc.non_finite_mask(pts, form["remove_nan"], form["remove_inf"])
        assert mask.tolist() == form["mask"], form
        if "expected" in form:
            assert np.array_equal(pts[mask], orc.f32(form["expected"]))


def test_oracle_neighbour_order_and_self_distance():
    # each point is its own first neighbour at distance 0; k' = min(k, N)
    p = np.array([[0, 0, 0], [3, 4, 0], [0, 0, 1]], np.float32)
    avg = orc.avg_distances(p, 20)
    want = np.array([(0 + 1 + 5) / 3, (0 + 5 + np.sqrt(np.float32(26))) / 3,
                     (0 + 1 + np.sqrt(np.float32(26))) / 3], np.float32)
    assert np.allclose(avg, want, rtol=1e-6)
    assert np.array_equal(orc.avg_distances(p, 1), np.zeros(3, np.float32))
    one = orc.statistical(p[:1], 20, 2.0)
    assert np.isnan(one["threshold"]) and not one["mask"].any()


# ---- 2. declared, exported, bound ------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from open3d_amd import _lib
    host_h = open(os.path.join(ROOT, "include", "o3d_mi355x_host.h")).read()
    so = C.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert name + "(" in host_h, name
        assert hasattr(so, name), name
        assert name in _lib.PROTOTYPES, name
    from open3d_amd import pointcloud, slac
    for fn in ("select_by_mask", "select_by_index", "remove_non_finite_points",
               "remove_duplicated_points", "remove_radius_outliers",
               "remove_statistical_outliers"):
        assert callable(getattr(pointcloud, fn)), fn
    assert callable(slac.preprocess_point_cloud)


# ---- 3. host guards ---------------------------------------------------------------
# Pointers that are never dereferenced: every call below must be refused by
# the argument checks, which come before any allocation, launch or copy. (The
# one row of the table that needs the data, a non-finite coordinate, is a GPU
# test.)
FAKE = C.c_void_p(0x1000)
NULL = C.c_void_p(0)


def _tables(n_ok=1, null_at=None):
    k = max(n_ok, 1)
    ins = (C.c_void_p * 9)(*[0x1000] * 9)
    outs = (C.c_void_p * 9)(*[0x2000] * 9)
    if null_at is not None:
        ins[null_at] = None
    widths = (C.c_int64 * 9)(*[12] * 9)
    return ins, widths, outs, k


def _L():
    from open3d_amd import _lib
    return _lib.lib()


def test_select_guards():
    L = _L()
    m = C.c_int64(-7)
    ins, widths, outs, _ = _tables()
    sel = L.o3dmi_pointcloud_select_by_mask
    assert sel(4, FAKE, 0, 1, ins, widths, outs, None, None) == INVALID_ARG
    assert sel(-1, FAKE, 0, 1, ins, widths, outs, C.byref(m), None) == \
        INVALID_ARG
    for bad in (0, 9, -1):
        assert sel(4, FAKE, 0, bad, ins, widths, outs, C.byref(m), None) == \
            INVALID_ARG
    assert sel(4, NULL, 0, 1, ins, widths, outs, C.byref(m), None) == \
        INVALID_ARG
    assert sel(4, FAKE, 0, 1, None, widths, outs, C.byref(m), None) == \
        INVALID_ARG
    assert sel(4, FAKE, 0, 1, ins, None, outs, C.byref(m), None) == INVALID_ARG
    assert sel(4, FAKE, 0, 1, ins, widths, None, C.byref(m), None) == \
        INVALID_ARG
    nulled, _, _, _ = _tables(null_at=1)
    assert sel(4, FAKE, 0, 2, nulled, widths, outs, C.byref(m), None) == \
        INVALID_ARG
    zero = (C.c_int64 * 9)(*[0] * 9)
    assert sel(4, FAKE, 0, 1, ins, zero, outs, C.byref(m), None) == INVALID_ARG
    idx = L.o3dmi_pointcloud_select_by_index
    assert idx(4, FAKE, 2, 0, 0, 1, ins, widths, outs, None, None) == \
        INVALID_ARG
    assert idx(-1, FAKE, 2, 0, 0, 1, ins, widths, outs, C.byref(m), None) == \
        INVALID_ARG
    assert idx(4, FAKE, -2, 0, 0, 1, ins, widths, outs, C.byref(m), None) == \
        INVALID_ARG
    assert idx(4, NULL, 2, 0, 0, 1, ins, widths, outs, C.byref(m), None) == \
        INVALID_ARG
    for bad in (0, 9):
        assert idx(4, FAKE, 2, 0, 0, bad, ins, widths, outs, C.byref(m),
                   None) == INVALID_ARG
    assert m.value == -7  # nothing was written
    # n == 0: an empty result, not an error
    assert sel(0, NULL, 0, 1, ins, widths, outs, C.byref(m), None) == 0
    assert m.value == 0


@pytest.mark.parametrize("dtype", [0, 1])
def test_filter_guards(dtype):
    L = _L()
    m = C.c_int64(-7)
    M = C.byref(m)
    nf = L.o3dmi_pointcloud_remove_non_finite_points
    assert nf(NULL, 4, dtype, 1, 1, FAKE, M, None) == INVALID_ARG
    assert nf(FAKE, 4, dtype, 1, 1, NULL, M, None) == INVALID_ARG
    assert nf(FAKE, 4, dtype, 1, 1, FAKE, None, None) == INVALID_ARG
    assert nf(FAKE, -1, dtype, 1, 1, FAKE, M, None) == INVALID_ARG
    dup = L.o3dmi_pointcloud_remove_duplicated_points
    assert dup(NULL, 4, dtype, FAKE, M, None) == INVALID_ARG
    assert dup(FAKE, 4, dtype, NULL, M, None) == INVALID_ARG
    assert dup(FAKE, 4, dtype, FAKE, None, None) == INVALID_ARG
    assert dup(FAKE, -1, dtype, FAKE, M, None) == INVALID_ARG
    rad = L.o3dmi_pointcloud_remove_radius_outliers
    assert rad(NULL, 4, dtype, 3, 0.5, FAKE, M, None) == INVALID_ARG
    assert rad(FAKE, 4, dtype, 3, 0.5, NULL, M, None) == INVALID_ARG
    assert rad(FAKE, 4, dtype, 3, 0.5, FAKE, None, None) == INVALID_ARG
    assert rad(FAKE, -1, dtype, 3, 0.5, FAKE, M, None) == INVALID_ARG
    assert rad(FAKE, 4, dtype, 0, 0.5, FAKE, M, None) == INVALID_ARG
    assert rad(FAKE, 4, dtype, 3, 0.0, FAKE, M, None) == INVALID_ARG
    assert rad(FAKE, 4, dtype, 3, -1.0, FAKE, M, None) == INVALID_ARG
    assert rad(FAKE, 4, dtype, 3, float("nan"), FAKE, M, None) == INVALID_ARG
    st = L.o3dmi_pointcloud_remove_statistical_outliers
    assert st(NULL, 4, dtype, 20, 2.0, FAKE, None, None, M, None) == \
        INVALID_ARG
    assert st(FAKE, 4, dtype, 20, 2.0, NULL, None, None, M, None) == \
        INVALID_ARG
    assert st(FAKE, 4, dtype, 20, 2.0, FAKE, None, None, None, None) == \
        INVALID_ARG
    assert st(FAKE, -1, dtype, 20, 2.0, FAKE, None, None, M, None) == \
        INVALID_ARG
    assert st(FAKE, 4, dtype, 0, 2.0, FAKE, None, None, M, None) == INVALID_ARG
    assert st(FAKE, 4, dtype, 20, 0.0, FAKE, None, None, M, None) == \
        INVALID_ARG
    assert st(FAKE, 4, dtype, 20, -2.0, FAKE, None, None, M, None) == \
        INVALID_ARG
    assert st(FAKE, 4, dtype, 65, 2.0, FAKE, None, None, M, None) == \
        UNSUPPORTED
    pre = L.o3dmi_slac_preprocess_point_cloud
    assert pre(NULL, None, 4, dtype, 0.05, 0, FAKE, FAKE, M, None) == \
        INVALID_ARG
    assert pre(FAKE, None, 4, dtype, 0.05, 0, NULL, FAKE, M, None) == \
        INVALID_ARG
    assert pre(FAKE, None, 4, dtype, 0.05, 0, FAKE, NULL, M, None) == \
        INVALID_ARG
    assert pre(FAKE, None, 4, dtype, 0.05, 0, FAKE, FAKE, None, None) == \
        INVALID_ARG
    assert pre(FAKE, None, -1, dtype, 0.05, 0, FAKE, FAKE, M, None) == \
        INVALID_ARG
    assert m.value == -7  # nothing was written
    # n == 0: an empty mask, m = 0, OK
    for call in (lambda: nf(NULL, 0, dtype, 1, 1, NULL, M, None),
                 lambda: dup(NULL, 0, dtype, NULL, M, None),
                 lambda: rad(NULL, 0, dtype, 3, 0.5, NULL, M, None),
                 lambda: st(NULL, 0, dtype, 20, 2.0, NULL, None, None, M,
                            None)):
        m.value = -7
        assert call() == 0 and m.value == 0


# ---- 4. the guard band of the statistical GPU tests --------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("size", orc.STAT_SIZES)
def test_statistical_inputs_keep_clear_of_the_threshold(size, dtype):
    """No point of any statistical test input has |avg_i - threshold| <=
    1e-9 * threshold, so a float64 tree sum and fsum agree on every mask bit.
    The two inputs for which that cannot hold (all avg_i equal, sums exact:
    see exactly_degenerate) are named as such."""
    for nb in orc.STAT_NB:
        for ratio in orc.STAT_RATIO:
            res = orc.stat_reference(size, dtype, nb, ratio)
            if orc.exactly_degenerate(res):
                assert nb == 1 or size in ("n1", "n2"), (size, nb)
                # (n1: the threshold is NaN and nothing is kept)
                assert res["mask"].all() == (size != "n1")
                continue
            assert orc.guard_band_clear(res), (size, nb, ratio)


def test_surface_input_has_outliers_on_both_sides():
    res = orc.stat_reference("surface", np.float32, 20, 2.0)
    n = res["mask"].shape[0]
    assert 0 < n <= 4096
    assert 10 <= (~res["mask"]).sum() < n // 4
    for dtype in (np.float32, np.float64):
        p, pair = orc.radius_cloud(dtype)
        assert pair.shape == (2,)
        d = p[pair[0]].astype(np.float64) - p[pair[1]].astype(np.float64)
        assert float(np.sqrt((d * d).sum())) == orc.RADIUS
        masks = [orc.radius_mask(p, nb, orc.RADIUS) for nb in orc.RADIUS_NB]
        assert masks[0].all() and not masks[2].all() and masks[2].any()
        assert not masks[1][pair].any()  # d2 == r2 is not a neighbour
