"""CPU checks (no GPU) of PointCloud smoothing, boundary detection and normal
orientation: the numpy oracle against the reference's own unit-cube vectors,
the new symbols in the headers and the library, the host guards, the two
tangent frames of the boundary test, and the caps the GPU tests rely on (how
many points their exclusion rules may leave out)."""
import ctypes as C
import os

import numpy as np
import pytest

import _pointcloud_smooth_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 7

HOST_NAMES = ("o3dmi_pointcloud_smooth_laplacian",
              "o3dmi_pointcloud_smooth_taubin",
              "o3dmi_pointcloud_smooth_mls",
              "o3dmi_pointcloud_smooth_bilateral",
              "o3dmi_pointcloud_compute_boundary_points",
              "o3dmi_pointcloud_normalize_normals",
              "o3dmi_pointcloud_orient_normals_to_align_with_direction",
              "o3dmi_pointcloud_orient_normals_towards_camera_location")
KERNEL_NAMES = ("o3dmi_pointcloud_boundary_from_neighbors",)


def _f64(rows):
    return np.array(rows, np.float64)


# ---- 1. the oracle against the reference's vectors ----------------------------
def test_oracle_laplacian_unit_cube():
    v = orc.reference_vectors()
    c = v["laplacian"]
    got = orc.smooth_laplacian(_f64(v["cube"]), c["iterations"], c["lambda"],
                               c["max_nn"], c["fixed"], np.float64)
    assert np.allclose(got, _f64(c["expected"]), rtol=c["rtol"],
                       atol=c["atol"])


def test_oracle_taubin_unit_cube():
    v = orc.reference_vectors()
    c = v["taubin"]
    got = orc.smooth_laplacian(_f64(v["cube"]), c["iterations"], c["lambda"],
                               c["max_nn"], c["fixed"], np.float64,
                               mu=c["mu"])
    assert np.allclose(got, _f64(c["expected"]), rtol=c["rtol"],
                       atol=c["atol"])


def test_oracle_mls_displaced_cube():
    c = orc.reference_vectors()["mls"]
    p = _f64(c["points"])
    idx, d2, counts = orc.mls_lists(p, c["radius"], c["max_nn"])
    got = orc.smooth_mls(p, None, idx, d2, counts, c["radius"], np.float64)
    assert got["fitted"].all()
    assert np.allclose(got["points"], _f64(c["expected"]), rtol=c["rtol"],
                       atol=c["atol"])


def test_oracle_bilateral_unit_cube():
    v = orc.reference_vectors()
    c = v["bilateral"]
    p = _f64(v["cube"])
    idx, d2, counts = orc.hybrid_lists(p, c["radius"], c["max_nn"])
    got = orc.smooth_bilateral(p, _f64(c["normals"]), idx, d2, counts,
                               c["sigma_s"], c["sigma_r"], np.float64)
    assert np.allclose(got, _f64(c["expected"]), rtol=c["rtol"],
                       atol=c["atol"])


def test_oracle_boundary_cases():
    v = orc.reference_vectors()
    assert v["empty"]["expected_rows"] == 0
    empty = np.zeros((0, 3), np.float32)
    assert orc.smooth_laplacian(empty, 10, 0.5, 20, False,
                                np.float32).shape == (0, 3)
    t = v["two_points"]
    p = np.array(t["points"], np.float32)
    for case in t["unchanged"]:
        if case["op"] == "mls":
            idx, d2, counts = orc.mls_lists(p, case["radius"], case["max_nn"])
            got = orc.smooth_mls(p, None, idx, d2, counts, case["radius"],
                                 np.float32)["points"]
        else:
            got = orc.smooth_laplacian(
                p, case["iterations"], 0.5, 20, False, np.float32,
                mu=-0.53 if case["op"] == "taubin" else None)
        assert np.allclose(got, p, rtol=t["rtol"], atol=t["atol"]), case
    assert len(t["throws"]) == 2
    for case in t["throws"]:
        assert case["sigma_s"] <= 0 or case["sigma_r"] <= 0


def test_oracle_self_entry_is_skipped_by_index_not_by_slot():
    # three copies of one point and one other: for copy 2 the list (k = 2)
    # is {0, 1}: its own index is absent and both entries count
    p = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1], [3, 1, 1]], np.float32)
    idx = orc.knn_lists(p, 2)[0]
    assert idx[2].tolist() == [0, 1]
    out = orc.laplacian_pass(p, idx, 0.5, np.float32)
    assert np.array_equal(out[:3], p[:3])
    assert out[3].tolist() == [2.0, 1.0, 1.0]


# ---- 2. declared, exported, bound ------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from open3d_amd import _lib
    host_h = open(os.path.join(ROOT, "include", "o3d_mi355x_host.h")).read()
    kern_h = open(os.path.join(ROOT, "include", "o3d_mi355x.h")).read()
    so = C.CDLL(_lib.SO_PATH)
    for names, text in ((HOST_NAMES, host_h), (KERNEL_NAMES, kern_h)):
        for name in names:
            assert name + "(" in text, name
            assert hasattr(so, name), name
            assert name in _lib.PROTOTYPES, name
    assert _lib.lib().o3dmi_abi_version() == 1
    from open3d_amd import pointcloud
    for fn in ("smooth_laplacian", "smooth_taubin", "smooth_mls",
               "smooth_bilateral", "compute_boundary_points",
               "normalize_normals", "orient_normals_to_align_with_direction",
               "orient_normals_towards_camera_location"):
        assert callable(getattr(pointcloud, fn)), fn


# ---- 3. host guards ---------------------------------------------------------------
# Pointers that are never dereferenced: every call is refused by the argument
# checks, which come before any allocation, launch or copy.
P, N, OUT, OUT2 = (C.c_void_p(0x100000), C.c_void_p(0x200000),
                   C.c_void_p(0x300000), C.c_void_p(0x400000))
NULL = C.c_void_p(0)


def _L():
    from open3d_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("dtype", [0, 1])
def test_smoothing_guards(dtype):
    L = _L()
    lap, tau = (L.o3dmi_pointcloud_smooth_laplacian,
                L.o3dmi_pointcloud_smooth_taubin)
    assert lap(P, 4, dtype, 1, 0.5, 64, 0, OUT, None) == UNSUPPORTED
    assert lap(P, 4, dtype, 1, 0.5, 64, 1, OUT, None) == UNSUPPORTED
    assert tau(P, 4, dtype, 1, 0.5, -0.53, 64, 0, OUT, None) == UNSUPPORTED
    assert lap(P, 4, dtype, 1, 0.5, 7, 0, P, None) == INVALID_ARG  # alias
    assert lap(P, 4, dtype, 1, 0.5, 7, 0, C.c_void_p(0x100000 + 8), None) == \
        INVALID_ARG
    assert lap(NULL, 4, dtype, 1, 0.5, 7, 0, OUT, None) == INVALID_ARG
    assert lap(P, 4, dtype, 1, 0.5, 7, 0, NULL, None) == INVALID_ARG
    assert lap(P, -1, dtype, 1, 0.5, 7, 0, OUT, None) == INVALID_ARG
    assert lap(P, 4, dtype, -1, 0.5, 7, 0, OUT, None) == INVALID_ARG
    assert lap(P, 4, 4, 1, 0.5, 7, 0, OUT, None) == INVALID_ARG  # Int32
    assert lap(NULL, 0, dtype, 1, 0.5, 7, 0, NULL, None) == 0
    assert tau(NULL, 0, dtype, 1, 0.5, -0.53, 7, 0, NULL, None) == 0
    mls = L.o3dmi_pointcloud_smooth_mls
    assert mls(P, None, 4, dtype, 0.1, 65, OUT, None, None) == UNSUPPORTED
    assert mls(P, None, 4, dtype, -1.0, 65, OUT, None, None) == UNSUPPORTED
    assert mls(P, None, 4, dtype, 0.1, 30, P, None, None) == INVALID_ARG
    assert mls(P, N, 4, dtype, 0.1, 30, OUT, N, None) == INVALID_ARG
    assert mls(P, N, 4, dtype, 0.1, 30, OUT, OUT, None) == INVALID_ARG
    assert mls(P, None, 4, dtype, 0.1, 30, OUT, OUT2, None) == INVALID_ARG
    assert mls(NULL, None, 4, dtype, 0.1, 30, OUT, None, None) == INVALID_ARG
    assert mls(NULL, None, 0, dtype, 0.1, 30, NULL, None, None) == 0
    bil = L.o3dmi_pointcloud_smooth_bilateral
    assert bil(P, N, 4, dtype, 0.1, 30, 0.0, 1.0, OUT, None) == INVALID_ARG
    assert bil(P, N, 4, dtype, 0.1, 30, 1.0, 0.0, OUT, None) == INVALID_ARG
    assert bil(P, N, 4, dtype, 0.1, 30, -1.0, 1.0, OUT, None) == INVALID_ARG
    assert bil(P, N, 4, dtype, 0.0, 30, 1.0, 1.0, OUT, None) == INVALID_ARG
    assert bil(P, NULL, 4, dtype, 0.1, 30, 1.0, 1.0, OUT, None) == INVALID_ARG
    assert bil(P, N, 4, dtype, 0.1, 30, 1.0, 1.0, N, None) == INVALID_ARG
    assert bil(P, N, 4, dtype, 0.1, 0, 1.0, 1.0, OUT, None) == INVALID_ARG
    assert bil(P, N, 4, dtype, 0.1, 65, 1.0, 1.0, OUT, None) == UNSUPPORTED
    # upstream returns the empty clone before it looks at the sigmas
    assert bil(NULL, NULL, 0, dtype, 0.1, 30, 0.0, 0.0, NULL, None) == 0
    m = C.c_int64(-7)
    M = C.byref(m)
    bnd = L.o3dmi_pointcloud_compute_boundary_points
    assert bnd(P, N, 4, dtype, 0.0, 30, 90.0, OUT, M, None) == INVALID_ARG
    assert bnd(P, NULL, 4, dtype, 0.1, 30, 90.0, OUT, M, None) == INVALID_ARG
    assert bnd(P, N, 4, dtype, 0.1, 30, 90.0, P, M, None) == INVALID_ARG
    assert bnd(P, N, 4, dtype, 0.1, 30, 90.0, OUT, None, None) == INVALID_ARG
    assert bnd(P, N, 4, dtype, 0.1, 65, 90.0, OUT, M, None) == UNSUPPORTED
    assert m.value == -7
    assert bnd(NULL, NULL, 0, dtype, 0.1, 30, 90.0, NULL, M, None) == 0
    assert m.value == 0
    seam = L.o3dmi_pointcloud_boundary_from_neighbors
    assert seam(P, N, OUT, OUT2, 4, 65, dtype, 90.0, OUT, None) == UNSUPPORTED
    assert seam(P, N, OUT, OUT2, 4, 0, dtype, 90.0, OUT, None) == INVALID_ARG
    assert seam(P, N, NULL, OUT2, 4, 30, dtype, 90.0, OUT, None) == \
        INVALID_ARG
    assert seam(P, N, OUT, NULL, 4, 30, dtype, 90.0, OUT, None) == INVALID_ARG
    nn, od, oc = (L.o3dmi_pointcloud_normalize_normals,
                  L.o3dmi_pointcloud_orient_normals_to_align_with_direction,
                  L.o3dmi_pointcloud_orient_normals_towards_camera_location)
    vec = (C.c_double * 3)(0, 0, 1)
    assert nn(NULL, 4, dtype, None) == INVALID_ARG
    assert nn(N, -1, dtype, None) == INVALID_ARG
    assert od(NULL, 4, dtype, vec, None) == INVALID_ARG
    assert od(N, 4, dtype, None, None) == INVALID_ARG
    assert oc(NULL, N, 4, dtype, vec, None) == INVALID_ARG
    assert oc(P, NULL, 4, dtype, vec, None) == INVALID_ARG
    assert oc(P, N, 4, dtype, None, None) == INVALID_ARG
    assert nn(NULL, 0, dtype, None) == 0


# ---- 4. the two tangent frames ------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_literal_frame_is_nan_on_z_normals_and_the_corrected_is_not(dtype):
    nrm = np.array([[0, 0, 1], [0, 0, -1]], dtype)
    u, v = orc.plane_frame(nrm, dtype, literal=True)
    assert np.isnan(u).any(1).all() and np.isnan(v).any(1).all()
    u, v = orc.plane_frame(nrm, dtype, literal=False)
    assert np.isfinite(u).all() and np.isfinite(v).all()
    # an orthonormal frame of the plane
    for r in range(2):
        assert abs(float(u[r] @ v[r])) < 1e-6 and abs(float(u[r] @ nrm[r])) < \
            1e-6
        assert abs(float(u[r] @ u[r]) - 1) < 1e-6
    # so on a floor the literal frame calls nothing a boundary point
    p, n, rim, interior = orc.grid_patch(12, dtype, tilt=False)
    idx, _, counts = orc.hybrid_lists(p, 2.5 * orc.SPACING, 30)
    lit, _ = orc.boundary(p, n, idx, counts, 90.0, dtype, literal=True)
    cor, _ = orc.boundary(p, n, idx, counts, 90.0, dtype, literal=False)
    assert not lit.any()
    assert cor[rim].all() and not cor[interior].any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_frames_agree_on_tilted_normals_away_from_the_threshold(dtype):
    p, n, rim, interior = orc.grid_patch(40, dtype, tilt=True)
    idx, _, counts = orc.hybrid_lists(p, 2.5 * orc.SPACING, 30)
    lit, _ = orc.boundary(p, n, idx, counts, 90.0, dtype, literal=True)
    cor, _ = orc.boundary(p, n, idx, counts, 90.0, dtype, literal=False)
    _, gap64 = orc.boundary(p, n, idx, counts, 90.0, np.float64)
    clear = np.abs(gap64 - np.pi / 2) > 1e-4
    assert (~clear).mean() <= 0.01
    assert np.array_equal(lit[clear], cor[clear])
    assert cor[rim].all() and not cor[interior].any()


# ---- 5. the caps of the GPU tests' exclusion rules ---------------------------------------
# The MLS inputs and parameters of the GPU tests are defined here, so that the
# 2 % cap is checked on the CPU for exactly what they run.
MLS_SCENES = [("plane", 65, 11), ("plane", 5003, 12), ("sphere", 5003, 13)]
RADIUS_ONLY_SCENE = ("plane", 1024, 21)


def mls_scene(kind, n, seed, dtype):
    if kind == "plane":
        side = int(np.ceil(np.sqrt(n)))
        p, nrm = orc.plane_patch(side, dtype, seed)
        return p[:n], nrm[:n]
    return orc.sphere_patch(n, dtype, seed)


def mls_input(kind, n, seed, dtype):
    """The scene with two isolated points (count < 3 in the hybrid and radius
    modes) whose normals are not unit vectors."""
    p, nrm = mls_scene(kind, n, seed, dtype)
    p[:2] += np.array([[9.0, 0, 0], [0, -9.0, 0]], dtype)
    nrm[:2] *= np.dtype(dtype).type(3.0)
    return p, nrm


def mls_params(kind, n):
    """(radius, max_nn) of every SmoothMLS call the GPU tests make on a
    scene: hybrid at each width, then KNN-only."""
    widths = (3, 30, 64) if n <= 65 or kind == "sphere" else (30,)
    return [(3 * orc.SPACING, w) for w in widths] + [(-1.0, 30)]


RADIUS_ONLY_PARAMS = [(5 * orc.SPACING, 0), (2 * orc.SPACING, -1)]
TINY_PARAMS = [(1.0, 30), (-1.0, 30), (1.0, 0), (-1.0, 2)]


def _left_out_share(p, radius, max_nn):
    idx, d2, counts = orc.mls_lists(p, radius, max_nn)
    res = orc.smooth_mls(p, None, idx, d2, counts, radius, np.float64)
    return float((res["fitted"] & (res["gap"] < 1e-3)).mean()), res


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,n,seed", MLS_SCENES)
def test_mls_scenes_leave_out_at_most_two_percent(kind, n, seed, dtype):
    p, _ = mls_input(kind, n, seed, dtype)
    for radius, max_nn in mls_params(kind, n):
        share, res = _left_out_share(p, radius, max_nn)
        assert share <= 0.02, (kind, n, radius, max_nn, share)
        if max_nn >= 30:
            assert res["fitted"].mean() > 0.9
        assert not res["fitted"][:2].any() or radius <= 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mls_radius_only_and_tiny_inputs_leave_out_at_most_two_percent(dtype):
    p, _ = mls_input(*RADIUS_ONLY_SCENE, dtype)
    for radius, max_nn in RADIUS_ONLY_PARAMS:
        share, res = _left_out_share(p, radius, max_nn)
        assert share <= 0.02, (radius, max_nn, share)
        assert res["fitted"].mean() > 0.9
    # two and three points
    for n in (2, 3):
        q = p[4:4 + n].copy()
        for radius, max_nn in TINY_PARAMS:
            share, res = _left_out_share(q, radius, max_nn)
            assert share <= 0.02, (n, radius, max_nn, share)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_boundary_scenes_keep_clear_of_the_threshold(dtype):
    for tilt in (False, True):
        p, n, rim, interior = orc.grid_patch(40, dtype, tilt)
        for max_nn in (2, 30, 64):
            idx, _, counts = orc.hybrid_lists(p, 2.5 * orc.SPACING, max_nn)
            _, gap = orc.boundary(p, n, idx, counts, 90.0, np.float64)
            assert (np.abs(gap - np.pi / 2) <= 1e-4).mean() <= 0.01
        assert sorted(counts[-4:].tolist()) == [1, 1, 2, 2]
    p, n = orc.sphere_shell(2000, dtype)
    idx, _, counts = orc.hybrid_lists(p, 0.2, 30)
    mask, gap = orc.boundary(p, n, idx, counts, 90.0, np.float64)
    assert not mask.any()
    assert (np.abs(gap - np.pi / 2) <= 1e-4).mean() <= 0.01
