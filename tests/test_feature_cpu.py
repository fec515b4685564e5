"""CPU checks of FPFH / feature correspondences: the numpy restatement
(tests/_fpfh_oracle.py) against hand-computed cases, and the new C ABI
symbols in the built library."""
import ctypes
import math

import numpy as np
import pytest

import _fpfh_oracle as fo

DTYPES = [np.float32, np.float64]


@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_feature_perpendicular_normals(dtype):
    # dp = x, n1 = z, n2 = y: no swap (both angles 0), v = dp x n1 = -y,
    # w = n1 x v = x, f1 = v . n2 = -1, f0 = atan2(w . n2, n1 . n2) = 0
    f = fo.pair_feature([0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], dtype)
    assert [float(x) for x in f] == [0.0, -1.0, 0.0, 1.0]
    assert fo.spfh_bins(*f[:3]) == (5, 0, 5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_feature_swap(dtype):
    # |angle2| = 0.6 > |angle1| = 0: the roles swap, dp flips, f2 = -angle2;
    # v = (-x) x (0.6, 0, 0.8) / 0.8 = y, w = (-0.8, 0, 0.6), f1 = 0,
    # f0 = atan2(0.6, 0.8)
    f = fo.pair_feature([0, 0, 0], [0, 0, 1], [2, 0, 0], [0.6, 0, 0.8], dtype)
    tol = 1e-6 if dtype == np.float32 else 1e-14
    assert abs(float(f[0]) - math.atan2(0.6, 0.8)) < tol
    assert abs(float(f[1])) < tol
    assert abs(float(f[2]) + 0.6) < tol
    assert float(f[3]) == 2.0
    # 11 (0.6435 + pi) / 2pi = 6.63, 11 / 2 = 5.5, 11 * 0.4 / 2 = 2.2
    assert fo.spfh_bins(*f[:3]) == (6, 5, 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_feature_degenerate(dtype):
    # zero distance
    assert [float(x) for x in fo.pair_feature(
        [1, 2, 3], [0, 0, 1], [1, 2, 3], [0, 1, 0], dtype)] == [0, 0, 0, 0]
    # normals parallel to the offset: v = 0
    assert [float(x) for x in fo.pair_feature(
        [0, 0, 0], [1, 0, 0], [3, 0, 0], [1, 0, 0], dtype)] == [0, 0, 0, 0]


def test_bin_clamping():
    assert fo.spfh_bins(math.pi, 1.0, 1.0) == (10, 10, 10)
    assert fo.spfh_bins(-math.pi, -1.0, -1.0) == (0, 0, 0)
    assert fo.spfh_bins(4.0, 1.5, -1.5) == (10, 10, 0)
    # just inside the top edge stays in bin 10, not clamped from 11
    assert fo.spfh_bins(math.pi - 1e-9, 1 - 1e-9, -1 + 1e-9) == (10, 10, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_five_point_planar_cloud_by_hand(dtype):
    """Five points on z = 0 with normals +z: every pair feature is
    (0, 0, 0, d) -> bins 5, 16, 27. Each SPFH row is 4 x 25 = 100 in those
    bins; the FPFH row is sum(100 / d2) * (100 / sum(100 / d2)) + 100 = 200
    there, 0 elsewhere."""
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [-1.5, 0.5, 0],
                    [0.3, -0.7, 0]], dtype)
    nrm = np.tile(np.array([0, 0, 1], dtype), (5, 1))
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    idx = np.argsort(d2, axis=1, kind="stable").astype(np.int32)
    dd = np.take_along_axis(d2, idx, 1).astype(dtype)
    counts = np.full(5, 5, np.int32)
    got = fo.fpfh_from_lists(pts, nrm, idx, dd, counts=counts)
    want = np.zeros((5, 33))
    want[:, [5, 16, 27]] = 200.0
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5)
    # counts of 1 (only the point itself): zero rows
    got1 = fo.fpfh_from_lists(pts, nrm, idx, dd, counts=np.ones(5, np.int32))
    assert not got1.any()


def test_radius_lists_and_csr_form_agree():
    rng = np.random.RandomState(3)
    pts = rng.uniform(-1, 1, (60, 3))
    nrm = rng.normal(size=(60, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    idx, dd, splits = fo.radius_lists(pts, 0.8)
    a = fo.fpfh_from_lists(pts, nrm, idx, dd, splits=splits)
    # the same lists padded
    w = int(np.diff(splits).max())
    pi = np.full((60, w), -1, np.int32)
    pd = np.zeros((60, w))
    for r in range(60):
        c = splits[r + 1] - splits[r]
        pi[r, :c] = idx[splits[r]:splits[r + 1]]
        pd[r, :c] = dd[splits[r]:splits[r + 1]]
    b = fo.fpfh_from_lists(pts, nrm, pi, pd, counts=np.diff(splits))
    assert np.array_equal(a, b)


def test_correspondence_restatement_ties_and_mutual():
    src = np.array([[0.0, 0.0], [1.0, 1.0], [5.0, 5.0]])
    tgt = np.array([[1.0, 1.0], [0.5, 0.5], [0.5, 0.5], [1.0, 1.0]])
    # row 0: 0.5 (index 1) and 0.5 (index 2) tie -> 1; row 1: indices 0, 3
    # tie at 0 -> 0
    pairs, fb = fo.correspondences(src, tgt)
    assert pairs.tolist() == [[0, 1], [1, 0], [2, 0]] and not fb
    # mutual: tgt 1 -> src 0, tgt 0 -> src 1 => rows 0, 1 survive
    pairs, fb = fo.correspondences(src, tgt, mutual_filter=True)
    assert pairs.tolist() == [[0, 1], [1, 0]] and not fb
    # ratio 0.9: 2 <= 0.9 * 3 -> fall back to all pairs
    pairs, fb = fo.correspondences(src, tgt, mutual_filter=True, ratio=0.9)
    assert pairs.shape == (3, 2) and fb


def test_feature_symbols_exported():
    from open3d_amd import _lib
    import __graft_entry__ as ge
    ge.build()
    so = ctypes.CDLL(_lib.SO_PATH)
    for name in ("o3dmi_fpfh_from_neighbors",
                 "o3dmi_registration_compute_fpfh_feature",
                 "o3dmi_registration_correspondences_from_features"):
        assert hasattr(so, name), name
        assert name in _lib.PROTOTYPES, name
