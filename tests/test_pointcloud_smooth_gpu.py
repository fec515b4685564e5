"""GPU tests of PointCloud smoothing, boundary detection and normal
orientation against the numpy oracle (tests/_pointcloud_smooth_oracle.py).

  * Laplacian / Taubin positions and the three normal calls: bit-exact.
  * MLS and bilateral: expf on the device and in numpy may differ in the last
    place, so the bound of a Float32 case is 4 x the largest deviation between
    the oracle in Float32 and the same oracle in Float64 on the same
    neighbour lists (the reference arithmetic's own spread; 4 allows one more
    rounding per transcendental and per divide than numpy's). Float64 cases
    use the reference tests' 1e-6 (MLS) and 1e-9 (bilateral) of the cloud's
    extent. MLS points whose two smallest covariance eigenvalues differ by
    less than 1e-3 of the largest are left out (at most 2 % of a case).
  * Boundary masks: exact wherever the largest gap (oracle, Float64) lies
    further than 1e-4 rad from the threshold (at most 1 % of a case inside).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _pointcloud_smooth_oracle as orc
from test_pointcloud_smooth_cpu import (MLS_SCENES, RADIUS_ONLY_PARAMS,
                                        RADIUS_ONLY_SCENE, TINY_PARAMS,
                                        mls_input, mls_params, mls_scene)

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, 7
DTYPES = [np.float32, np.float64]
O3DMI = {np.float32: 0, np.float64: 1}


def _pc():
    from open3d_amd import pointcloud
    return pointcloud


def _lib():
    from open3d_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(got, want, what=""):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, what
    if g.tobytes() != want.tobytes():
        bad = np.nonzero((g != want).any(-1) if g.ndim > 1 else g != want)[0]
        raise AssertionError("%s: %d rows differ, first %d: %r != %r" % (
            what, bad.size, bad[0], g[bad[0]], want[bad[0]]))


# ---- golden vectors (Float64, the reference tests' tolerances) ---------------------
def test_reference_unit_cube_vectors():
    v = orc.reference_vectors()
    pc = _pc()
    cube = {"positions": _dev(np.array(v["cube"], np.float64))}
    c = v["laplacian"]
    got = pc.smooth_laplacian(cube, c["iterations"], c["lambda"], c["max_nn"],
                              c["fixed"])["positions"].cpu().numpy()
    assert np.allclose(got, np.array(c["expected"]), rtol=c["rtol"],
                       atol=c["atol"])
    c = v["taubin"]
    got = pc.smooth_taubin(cube, c["iterations"], c["lambda"], c["mu"],
                           c["max_nn"], c["fixed"])["positions"].cpu().numpy()
    assert np.allclose(got, np.array(c["expected"]), rtol=c["rtol"],
                       atol=c["atol"])
    c = v["mls"]
    got = pc.smooth_mls({"positions": _dev(np.array(c["points"], np.float64))},
                        c["radius"], c["max_nn"])["positions"].cpu().numpy()
    assert np.allclose(got, np.array(c["expected"]), rtol=c["rtol"],
                       atol=c["atol"])
    c = v["bilateral"]
    with_n = dict(cube, normals=_dev(np.array(c["normals"], np.float64)))
    got = pc.smooth_bilateral(with_n, c["radius"], c["max_nn"], c["sigma_s"],
                              c["sigma_r"])["positions"].cpu().numpy()
    assert np.allclose(got, np.array(c["expected"]), rtol=c["rtol"],
                       atol=c["atol"])


def test_reference_boundary_cases():
    v = orc.reference_vectors()
    pc = _pc()
    empty = {"positions": torch.empty((0, 3), dtype=torch.float32,
                                      device="cuda")}
    for out in (pc.smooth_mls(empty), pc.smooth_laplacian(empty),
                pc.smooth_taubin(empty), pc.smooth_bilateral(empty)):
        assert out["positions"].shape == (v["empty"]["expected_rows"], 3)
    t = v["two_points"]
    p = np.array(t["points"], np.float32)
    two = {"positions": _dev(p)}
    for case in t["unchanged"]:
        if case["op"] == "mls":
            got = pc.smooth_mls(two, case["radius"], case["max_nn"])
        elif case["op"] == "laplacian":
            got = pc.smooth_laplacian(two, case["iterations"])
        else:
            got = pc.smooth_taubin(two, case["iterations"])
        assert np.allclose(got["positions"].cpu().numpy(), p, rtol=t["rtol"],
                           atol=t["atol"]), case
    for case in t["throws"]:
        with pytest.raises(ValueError, match="Sigma values must be positive"):
            pc.smooth_bilateral(two, case["radius"], case["max_nn"],
                                case["sigma_s"], case["sigma_r"])


# ---- Laplacian / Taubin: bit-exact ---------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 8, 63, 64, 65])
def test_laplacian_small_sizes_bit_exact(n, dtype):
    p = orc.laplacian_cloud(n, dtype)
    cloud = {"positions": _dev(p)}
    for max_nn in (1, 7, 30, 63):
        for fixed in (False, True):
            for iterations in (1, 3):
                want = orc.smooth_laplacian(p, iterations, 0.5, max_nn, fixed,
                                            dtype)
                got = _pc().smooth_laplacian(cloud, iterations, 0.5, max_nn,
                                             fixed)["positions"]
                _same_bits(got, want, "laplacian %r" % ((n, max_nn, fixed,
                                                         iterations),))
    for max_nn in (7, 63):
        for fixed in (False, True):
            for iterations in (1, 3):
                want = orc.smooth_laplacian(p, iterations, 0.5, max_nn, fixed,
                                            dtype, mu=-0.53)
                got = _pc().smooth_taubin(cloud, iterations, 0.5, -0.53,
                                          max_nn, fixed)["positions"]
                _same_bits(got, want, "taubin %r" % ((n, max_nn, fixed,
                                                      iterations),))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fixed", [False, True])
def test_laplacian_many_blocks_bit_exact(fixed, dtype):
    p = orc.laplacian_cloud(5003, dtype)
    cloud = {"positions": _dev(p)}
    want = orc.smooth_laplacian(p, 1, 0.5, 30, fixed, dtype)
    got = _pc().smooth_laplacian(cloud, 1, 0.5, 30, fixed)["positions"]
    _same_bits(got, want, "laplacian")
    want = orc.smooth_laplacian(p, 1, 0.5, 30, fixed, dtype, mu=-0.53)
    got = _pc().smooth_taubin(cloud, 1, 0.5, -0.53, 30, fixed)["positions"]
    _same_bits(got, want, "taubin")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,n", [("dups", 200), ("offset", 500)])
def test_laplacian_duplicates_and_offset_bit_exact(kind, n, dtype):
    """dups: 70 copies of one point, so with max_nn = 63 the self entry of
    the later copies is absent from their 64-wide list; offset: 1000 m."""
    p = orc.laplacian_cloud(n, dtype, kind)
    cloud = {"positions": _dev(p)}
    if kind == "dups":
        idx = orc.knn_lists(p, 64)[0]
        assert not (idx[70] == 70).any() and (idx[5] == 5).any()
    for max_nn in (7, 63):
        for fixed in (False, True):
            want = orc.smooth_laplacian(p, 3, 0.5, max_nn, fixed, dtype)
            got = _pc().smooth_laplacian(cloud, 3, 0.5, max_nn,
                                         fixed)["positions"]
            _same_bits(got, want, "%s %r" % (kind, (max_nn, fixed)))
    want = orc.smooth_laplacian(p, 2, 0.5, 30, False, dtype, mu=-0.53)
    got = _pc().smooth_taubin(cloud, 2, 0.5, -0.53, 30, False)["positions"]
    _same_bits(got, want, kind + " taubin")


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_and_table_forms_give_the_same_bits(dtype):
    for n, max_nn in ((65, 63), (1500, 20)):
        cloud = {"positions": _dev(orc.laplacian_cloud(n, dtype))}
        fused = _pc().smooth_laplacian(cloud, 1, 0.5, max_nn, False)
        table = _pc().smooth_laplacian(cloud, 1, 0.5, max_nn, True)
        assert torch.equal(fused["positions"], table["positions"])


# ---- MLS and bilateral: within the reference arithmetic's own spread ---------------
def _extent(p):
    return float((p.max(0) - p.min(0)).max())


def _mls_check(p, nrm, radius, max_nn, dtype):
    idx, d2, counts = orc.mls_lists(p, radius, max_nn)
    ref = orc.smooth_mls(p, nrm, idx, d2, counts, radius, dtype)
    ref64 = orc.smooth_mls(p, nrm, idx, d2, counts, radius, np.float64)
    keep = ~(ref64["fitted"] & (ref64["gap"] < 1e-3))
    assert (~keep).mean() <= 0.02
    cloud = {"positions": _dev(p)}
    if nrm is not None:
        cloud["normals"] = _dev(nrm)
    out = _pc().smooth_mls(cloud, radius, max_nn)
    got = out["positions"].cpu().numpy()
    assert got.dtype == p.dtype
    if dtype == np.float32:
        bound = 4 * float(np.abs(ref["points"][keep].astype(np.float64) -
                                 ref64["points"][keep]).max())
    else:
        bound = 1e-6 * _extent(p)
    err = float(np.abs(got[keep].astype(np.float64) -
                       ref["points"][keep].astype(np.float64)).max())
    print("mls n=%d radius=%g max_nn=%d %s: err %.3g bound %.3g left out %d"
          % (p.shape[0], radius, max_nn, np.dtype(dtype).name, err, bound,
             int((~keep).sum())))
    assert err <= bound
    # points that are not fitted stay where they are, bit for bit
    stay = ~ref64["fitted"]
    assert got[stay].tobytes() == p[stay].tobytes()
    if nrm is None:
        assert "normals" not in out
        return
    gn = out["normals"].cpu().numpy().astype(np.float64)
    few = counts < 3
    assert gn[few].astype(dtype).tobytes() == ref["normals"][few].tobytes()
    fit = keep & ref64["fitted"]
    if not fit.any():
        return
    cos = np.abs((gn[fit] * ref["normals"][fit].astype(np.float64)).sum(1))
    assert cos.min() >= 1 - 1e-6
    # the library's sign rule: last non-zero component positive
    assert (gn[fit][:, 2] > 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,n,seed", MLS_SCENES)
def test_mls_hybrid_and_knn(kind, n, seed, dtype):
    # two isolated points: count < 3 in the hybrid mode. Inputs and
    # parameters are those whose 2 % cap the CPU test checks.
    p, nrm = mls_input(kind, n, seed, dtype)
    params = mls_params(kind, n)
    for radius, max_nn in params[:-1]:
        _mls_check(p, nrm, radius, max_nn, dtype)
    _mls_check(p, None, 3 * orc.SPACING, 30, dtype)
    assert params[-1] == (-1.0, 30)
    _mls_check(p, nrm if n <= 65 else None, -1.0, 30, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mls_radius_only_and_tiny_clouds(dtype):
    p, nrm = mls_input(*RADIUS_ONLY_SCENE, dtype)
    # rows wider than one wave: the radius-only mode has no limit
    idx, _, counts = orc.radius_lists(p, RADIUS_ONLY_PARAMS[0][0])
    assert counts.max() > 64 and counts.min() == 1
    _mls_check(p, nrm, *RADIUS_ONLY_PARAMS[0], dtype)
    _mls_check(p, None, *RADIUS_ONLY_PARAMS[1], dtype)
    for n in (2, 3):
        q, qn = p[4:4 + n].copy(), nrm[4:4 + n] * dtype(2.0)
        for radius, max_nn in TINY_PARAMS:
            _mls_check(q, qn, radius, max_nn, dtype)
    # both <= 0: a copy
    out = _pc().smooth_mls({"positions": _dev(p)}, -1.0, 0)
    _same_bits(out["positions"], p)


def _bilateral_check(p, nrm, radius, max_nn, sigma_s, sigma_r, dtype):
    idx, d2, counts = orc.hybrid_lists(p, radius, max_nn)
    ref = orc.smooth_bilateral(p, nrm, idx, d2, counts, sigma_s, sigma_r,
                               dtype)
    ref64 = orc.smooth_bilateral(p, nrm, idx, d2, counts, sigma_s, sigma_r,
                                 np.float64)
    got = _pc().smooth_bilateral(
        {"positions": _dev(p), "normals": _dev(nrm)}, radius, max_nn, sigma_s,
        sigma_r)["positions"].cpu().numpy()
    if dtype == np.float32:
        bound = 4 * float(np.abs(ref.astype(np.float64) - ref64).max())
    else:
        bound = 1e-9 * _extent(p)
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print("bilateral n=%d max_nn=%d %s: err %.3g bound %.3g" % (
        p.shape[0], max_nn, np.dtype(dtype).name, err, bound))
    assert err <= bound
    stay = (counts <= 1) | ((nrm.astype(np.float64) ** 2).sum(1) == 0)
    assert got[stay].tobytes() == p[stay].tobytes()
    if (~stay).any():
        assert (got[~stay] != p[~stay]).any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,n,seed", MLS_SCENES)
def test_bilateral(kind, n, seed, dtype):
    p, nrm = mls_scene(kind, n, seed, dtype)
    p[:2] += np.array([[9.0, 0, 0], [0, -9.0, 0]], dtype)  # count == 1
    nrm = nrm * dtype(2.5)  # the kernel normalises
    nrm[5] = 0              # a zero normal stays
    for max_nn in ((3, 30, 64) if n <= 65 or kind == "sphere" else (30,)):
        _bilateral_check(p, nrm, 3 * orc.SPACING, max_nn, 2 * orc.SPACING,
                         orc.SPACING, dtype)
    for n_small in (2, 3):
        _bilateral_check(p[6:6 + n_small].copy(), nrm[6:6 + n_small].copy(),
                         1.0, 30, 0.1, 0.1, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_table_forms_of_mls_and_bilateral_give_the_fused_bits(dtype):
    """The chain a seam-by-seam port would run (tools/bench_pointcloud_
    smooth.py): the existing hybrid search into a table, then the internal
    table-reading kernel -- the same per-point body, so the same bytes."""
    p, nrm = mls_input("plane", 1500, 71, dtype)
    n, max_nn, radius = p.shape[0], 30, 3 * orc.SPACING
    L = _lib()
    fn = L.lib().o3dmi_internal_pointcloud_smooth_from_neighbors
    assert fn.argtypes == L.INTERNAL_PROTOTYPES[
        "o3dmi_internal_pointcloud_smooth_from_neighbors"][1]
    P, N = _dev(p), _dev(nrm)
    tab = torch.empty((n, max_nn), dtype=torch.int32, device="cuda")
    d2 = torch.empty((n, max_nn), dtype=P.dtype, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    index = C.c_void_p()
    L.check(L.lib().o3dmi_nns_create(L.ptr(P), n, O3DMI[dtype],
                                     C.c_double(radius), None,
                                     C.byref(index)), "nns_create")
    try:
        L.check(L.lib().o3dmi_nns_hybrid_search(
            index, L.ptr(P), n, max_nn, L.ptr(tab), L.ptr(d2), L.ptr(cnt),
            None), "hybrid_search")
        mls_p, mls_n, bil_p = P.clone(), N.clone(), P.clone()
        L.check(fn(1, L.ptr(P), None, L.ptr(tab), L.ptr(d2), L.ptr(cnt), n,
                   max_nn, O3DMI[dtype], radius, 0.0, L.ptr(mls_p),
                   L.ptr(mls_n), None, None), "table mls")
        L.check(fn(2, L.ptr(P), L.ptr(N), L.ptr(tab), L.ptr(d2), L.ptr(cnt),
                   n, max_nn, O3DMI[dtype], 0.1, 0.05, L.ptr(bil_p), None,
                   None, None), "table bilateral")
        torch.cuda.synchronize()
    finally:
        L.lib().o3dmi_nns_destroy(index)
    cloud = {"positions": P, "normals": N}
    fused = _pc().smooth_mls(cloud, radius, max_nn)
    assert torch.equal(fused["positions"], mls_p)
    assert torch.equal(fused["normals"], mls_n)
    fused = _pc().smooth_bilateral(cloud, radius, max_nn, 0.1, 0.05)
    assert torch.equal(fused["positions"], bil_p)
    assert not torch.equal(bil_p, P)


def test_bilateral_without_normals_estimates_them_first():
    p, _ = mls_scene("plane", 400, 31, np.float32)
    cloud = {"positions": _dev(p), "label": torch.arange(400, device="cuda")}
    out = _pc().smooth_bilateral(cloud, 3 * orc.SPACING, 30, 0.1, 0.05)
    nrm = torch.empty_like(cloud["positions"])
    L = _lib()
    L.check(L.lib().o3dmi_pointcloud_estimate_normals(
        L.ptr(cloud["positions"]), 400, 0, 30, C.c_double(-1.0), L.ptr(nrm), 0,
        None), "estimate_normals")
    assert torch.equal(out["normals"], nrm)
    want = _pc().smooth_bilateral(dict(cloud, normals=nrm), 3 * orc.SPACING,
                                  30, 0.1, 0.05)
    assert torch.equal(out["positions"], want["positions"])
    assert out["label"] is cloud["label"]


# ---- boundary ----------------------------------------------------------------------------
def _boundary_check(p, nrm, radius, max_nn, dtype, literal_too=False):
    idx, _, counts = orc.hybrid_lists(p, radius, max_nn)
    want, _ = orc.boundary(p, nrm, idx, counts, 90.0, dtype)
    _, gap64 = orc.boundary(p, nrm, idx, counts, 90.0, np.float64)
    clear = np.abs(gap64 - np.pi / 2) > 1e-4
    assert (~clear).mean() <= 0.01
    cloud = {"positions": _dev(p), "normals": _dev(nrm),
             "id": torch.arange(p.shape[0], device="cuda")}
    sub, mask = _pc().compute_boundary_points(cloud, radius, max_nn, 90.0)
    assert mask.dtype == torch.bool
    got = mask.cpu().numpy()
    assert np.array_equal(got[clear], want[clear])
    assert np.array_equal(sub["id"].cpu().numpy(), np.nonzero(got)[0])
    _same_bits(sub["positions"], p[got])
    if literal_too:
        lit, _ = orc.boundary(p, nrm, idx, counts, 90.0, dtype, literal=True)
        assert np.array_equal(got[clear], lit[clear])
    # the kernel seam on the existing hybrid search's table: the same mask
    L = _lib()
    n = p.shape[0]
    P, N = cloud["positions"], cloud["normals"]
    index = C.c_void_p()
    L.check(L.lib().o3dmi_nns_create(L.ptr(P), n, O3DMI[dtype],
                                     C.c_double(radius), None,
                                     C.byref(index)), "nns_create")
    try:
        tab = torch.empty((n, max_nn), dtype=torch.int32, device="cuda")
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        L.check(L.lib().o3dmi_nns_hybrid_search(
            index, L.ptr(P), n, max_nn, L.ptr(tab), None, L.ptr(cnt), None),
            "hybrid_search")
        seam = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        L.check(L.lib().o3dmi_pointcloud_boundary_from_neighbors(
            L.ptr(P), L.ptr(N), L.ptr(tab), L.ptr(cnt), n, max_nn,
            O3DMI[dtype], C.c_double(90.0), L.ptr(seam), None), "seam")
        torch.cuda.synchronize()
    finally:
        L.lib().o3dmi_nns_destroy(index)
    assert np.array_equal(seam.cpu().numpy().astype(bool), got)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tilt", [False, True])
def test_boundary_grid_patch(tilt, dtype):
    p, nrm, rim, interior = orc.grid_patch(40, dtype, tilt)
    got = _boundary_check(p, nrm, 2.5 * orc.SPACING, 30, dtype,
                          literal_too=tilt)
    # the rim and only the rim; the points with count 1 or 2 ...
    assert got[rim].all() and not got[interior].any()
    assert got[-4:].tolist() == [False, False, True, True]
    for max_nn in (2, 64):
        _boundary_check(p, nrm, 2.5 * orc.SPACING, max_nn, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary_closed_sphere_has_none(dtype):
    p, nrm = orc.sphere_shell(2000, dtype)
    got = _boundary_check(p, nrm, 0.2, 30, dtype)
    assert not got.any()


# ---- normals: bit-exact --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 65, 5003])
def test_normal_calls_bit_exact(n, dtype):
    rng = np.random.RandomState(n)
    p = rng.uniform(-2, 2, (n, 3)).astype(dtype)
    nrm = rng.normal(size=(n, 3)).astype(dtype) * dtype(3)
    direction = np.array([0.5, -0.25, 0.5])
    camera = np.array([0.25, -1.5, 3.0])
    nrm[0] = 0                       # a zero normal
    if n > 3:
        nrm[1] = 0
        p[1] = camera.astype(dtype)  # ... at the camera location
        nrm[2] = np.array([1, 2, 0], dtype)  # orthogonal to the direction
        nrm[3] = np.array([0, 0, -1], dtype)
        assert float(nrm[2].astype(np.float64) @ direction) == 0.0
    cloud = {"positions": _dev(p), "normals": _dev(nrm),
             "colors": torch.zeros((n, 3), dtype=torch.uint8, device="cuda")}
    pc = _pc()
    out = pc.normalize_normals(cloud)
    _same_bits(out["normals"], orc.normalize_normals(nrm, dtype), "normalize")
    assert out["colors"] is cloud["colors"]
    _same_bits(cloud["normals"], nrm, "input untouched")
    out = pc.orient_normals_to_align_with_direction(cloud, direction)
    _same_bits(out["normals"], orc.orient_to_direction(nrm, direction, dtype),
               "direction")
    out = pc.orient_normals_towards_camera_location(cloud, camera)
    want = orc.orient_to_camera(p, nrm, camera, dtype)
    _same_bits(out["normals"], want, "camera")
    if n > 3:
        assert want[1].tolist() == [0, 0, 1]


# ---- errors: the return code, and the outputs untouched ------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_errors_leave_the_outputs_untouched(dtype):
    L = _lib()
    lib = L.lib()
    dt = O3DMI[dtype]
    n = 100
    p, nrm = mls_scene("plane", n, 41, dtype)
    P, N = _dev(p), _dev(nrm)
    bad = p.copy()
    bad[17, 1] = np.nan
    BAD = _dev(bad)
    inf = p.copy()
    inf[3, 2] = np.inf
    INF = _dev(inf)
    t = torch.float32 if dtype == np.float32 else torch.float64

    def sentinel():
        return torch.full((n, 3), -12345.5, dtype=t, device="cuda")

    def untouched(*outs):
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == (-12345.5 if o.dtype != torch.uint8
                               else 0xA5)).all())

    m = C.c_int64(-7)
    for pts in (BAD, INF):
        o, o2 = sentinel(), sentinel()
        for fixed in (0, 1):
            assert lib.o3dmi_pointcloud_smooth_laplacian(
                L.ptr(pts), n, dt, 2, 0.5, 7, fixed, L.ptr(o), None) == \
                INVALID_ARG
            assert lib.o3dmi_pointcloud_smooth_taubin(
                L.ptr(pts), n, dt, 2, 0.5, -0.53, 7, fixed, L.ptr(o),
                None) == INVALID_ARG
        for radius, max_nn in ((0.1, 30), (-1.0, 30), (0.1, 0)):
            assert lib.o3dmi_pointcloud_smooth_mls(
                L.ptr(pts), L.ptr(N), n, dt, radius, max_nn, L.ptr(o),
                L.ptr(o2), None) == INVALID_ARG
        assert lib.o3dmi_pointcloud_smooth_bilateral(
            L.ptr(pts), L.ptr(N), n, dt, 0.1, 30, 0.1, 0.1, L.ptr(o),
            None) == INVALID_ARG
        mask = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        assert lib.o3dmi_pointcloud_compute_boundary_points(
            L.ptr(pts), L.ptr(N), n, dt, 0.1, 30, 90.0, L.ptr(mask),
            C.byref(m), None) == INVALID_ARG
        untouched(o, o2, mask)
        assert m.value == -7
    o, o2 = sentinel(), sentinel()
    mask = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    calls = [
        (UNSUPPORTED, lambda: lib.o3dmi_pointcloud_smooth_laplacian(
            L.ptr(P), n, dt, 1, 0.5, 64, 0, L.ptr(o), None)),
        (UNSUPPORTED, lambda: lib.o3dmi_pointcloud_smooth_taubin(
            L.ptr(P), n, dt, 1, 0.5, -0.53, 64, 1, L.ptr(o), None)),
        (UNSUPPORTED, lambda: lib.o3dmi_pointcloud_smooth_mls(
            L.ptr(P), L.ptr(N), n, dt, 0.1, 65, L.ptr(o), L.ptr(o2), None)),
        (UNSUPPORTED, lambda: lib.o3dmi_pointcloud_smooth_mls(
            L.ptr(P), L.ptr(N), n, dt, -1.0, 65, L.ptr(o), L.ptr(o2), None)),
        (UNSUPPORTED, lambda: lib.o3dmi_pointcloud_smooth_bilateral(
            L.ptr(P), L.ptr(N), n, dt, 0.1, 65, 0.1, 0.1, L.ptr(o), None)),
        (UNSUPPORTED, lambda: lib.o3dmi_pointcloud_compute_boundary_points(
            L.ptr(P), L.ptr(N), n, dt, 0.1, 65, 90.0, L.ptr(mask), C.byref(m),
            None)),
        (INVALID_ARG, lambda: lib.o3dmi_pointcloud_smooth_bilateral(
            L.ptr(P), L.ptr(N), n, dt, 0.1, 30, 0.0, 0.1, L.ptr(o), None)),
        (INVALID_ARG, lambda: lib.o3dmi_pointcloud_smooth_bilateral(
            L.ptr(P), L.ptr(N), n, dt, 0.1, 30, 0.1, -1.0, L.ptr(o), None)),
        (INVALID_ARG, lambda: lib.o3dmi_pointcloud_smooth_bilateral(
            L.ptr(P), L.ptr(N), n, dt, 0.0, 30, 0.1, 0.1, L.ptr(o), None)),
        (INVALID_ARG, lambda: lib.o3dmi_pointcloud_smooth_bilateral(
            L.ptr(P), None, n, dt, 0.1, 30, 0.1, 0.1, L.ptr(o), None)),
        (INVALID_ARG, lambda: lib.o3dmi_pointcloud_compute_boundary_points(
            L.ptr(P), L.ptr(N), n, dt, -1.0, 30, 90.0, L.ptr(mask),
            C.byref(m), None)),
        (INVALID_ARG, lambda: lib.o3dmi_pointcloud_compute_boundary_points(
            L.ptr(P), None, n, dt, 0.1, 30, 90.0, L.ptr(mask), C.byref(m),
            None)),
    ]
    for code, call in calls:
        assert call() == code
    untouched(o, o2, mask)
    assert m.value == -7
    # an output that aliases an input: the input keeps its contents
    keep_p, keep_n = P.clone(), N.clone()
    assert lib.o3dmi_pointcloud_smooth_laplacian(
        L.ptr(P), n, dt, 1, 0.5, 7, 0, L.ptr(P), None) == INVALID_ARG
    assert lib.o3dmi_pointcloud_smooth_mls(
        L.ptr(P), L.ptr(N), n, dt, 0.1, 30, L.ptr(o), L.ptr(N), None) == \
        INVALID_ARG
    assert lib.o3dmi_pointcloud_smooth_bilateral(
        L.ptr(P), L.ptr(N), n, dt, 0.1, 30, 0.1, 0.1, L.ptr(N), None) == \
        INVALID_ARG
    untouched(o)
    assert torch.equal(P, keep_p) and torch.equal(N, keep_n)
    with pytest.raises(ValueError):
        _pc().compute_boundary_points({"positions": P}, 0.1)
    with pytest.raises(ValueError):
        _pc().orient_normals_to_align_with_direction({"positions": P})


# ---- copies, carried attributes, run to run ----------------------------------------------
def test_copies_and_carried_attributes():
    p, nrm = mls_scene("plane", 300, 51, np.float32)
    cloud = {"positions": _dev(p), "normals": _dev(nrm),
             "colors": torch.randint(0, 255, (300, 3), dtype=torch.uint8,
                                     device="cuda")}
    pc = _pc()
    for out in (pc.smooth_laplacian(cloud, 0), pc.smooth_laplacian(cloud, 3,
                                                                   0.5, 0),
                pc.smooth_taubin(cloud, 0), pc.smooth_taubin(cloud, 2, 0.5,
                                                             -0.53, -1)):
        _same_bits(out["positions"], p)
        assert out["positions"].data_ptr() != cloud["positions"].data_ptr()
        assert out["colors"] is cloud["colors"]
        assert out["normals"] is cloud["normals"]
    out = pc.smooth_mls(cloud, 3 * orc.SPACING, 30)
    assert set(out) == set(cloud) and out["colors"] is cloud["colors"]
    assert out["normals"] is not cloud["normals"]
    _same_bits(cloud["positions"], p, "input untouched")
    _same_bits(cloud["normals"], nrm, "input untouched")


@pytest.mark.parametrize("dtype", DTYPES)
def test_run_to_run(dtype):
    p, nrm = mls_scene("sphere", 3000, 61, dtype)
    cloud = {"positions": _dev(p), "normals": _dev(nrm)}
    pc = _pc()
    r = 3 * orc.SPACING
    ops = [lambda: pc.smooth_laplacian(cloud, 2, 0.5, 20, False),
           lambda: pc.smooth_laplacian(cloud, 2, 0.5, 20, True),
           lambda: pc.smooth_taubin(cloud, 2, 0.5, -0.53, 20, False),
           lambda: pc.smooth_mls(cloud, r, 30),
           lambda: pc.smooth_mls(cloud, -1.0, 30),
           lambda: pc.smooth_mls(cloud, r, 0),
           lambda: pc.smooth_bilateral(cloud, r, 30, r, r),
           lambda: pc.normalize_normals(cloud),
           lambda: pc.orient_normals_to_align_with_direction(cloud, (1, 2, 3)),
           lambda: pc.orient_normals_towards_camera_location(cloud,
                                                             (1, 2, 3))]
    for k, op in enumerate(ops):
        a, b = op(), op()
        for key in ("positions", "normals"):
            assert torch.equal(a[key], b[key]), (k, key)
    (_, m1), (_, m2) = (pc.compute_boundary_points(cloud, r, 30),
                        pc.compute_boundary_points(cloud, r, 30))
    assert torch.equal(m1, m2)
