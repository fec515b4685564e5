"""GPU tests of the PointCloud selection / filter family against the numpy
oracle (tests/_pointcloud_filter_oracle.py): masks and compacted rows are
exact, the per-point average distances bit-exact, the cloud statistics within
the float64 summation bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import _pointcloud_filter_oracle as orc

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, 7
SCAN_TILE = 1024 * 8  # scan.hip: kScanBlock x kScanItems


def _pc():
    from open3d_amd import pointcloud
    return pointcloud


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cloud(n, seed):
    """Four attributes: rows of 12, 24, 3 and 4 bytes."""
    rng = np.random.RandomState(seed)
    return {"positions": rng.normal(size=(n, 3)).astype(np.float32),
            "normals64": rng.normal(size=(n, 3)),
            "colors": rng.randint(0, 256, (n, 3)).astype(np.uint8),
            "label": rng.randint(-9, 9, (n,)).astype(np.int32)}


def _same_rows(got, want):
    assert set(got) == set(want)
    for k in want:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, k
        assert g.tobytes() == want[k].tobytes(), k


# ---- select ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, SCAN_TILE + 1])
def test_select_by_mask_sizes(n):
    cloud = _cloud(n, n)
    mask = np.random.RandomState(n + 1).rand(n) < 0.5
    dev = {k: _dev(v) for k, v in cloud.items()}
    for invert in (False, True):
        got, _ = _pc().select_by_mask(dev, _dev(mask), invert)
        _same_rows(got, orc.select_by_mask(cloud, mask, invert))


@pytest.mark.parametrize("kind", ["true", "false", "alternating", "random"])
def test_select_by_mask_patterns(kind):
    n = 5003
    cloud = _cloud(n, 5)
    mask = {"true": np.ones(n, bool), "false": np.zeros(n, bool),
            "alternating": np.arange(n) % 2 == 0,
            "random": np.random.RandomState(9).rand(n) < 0.3}[kind]
    dev = {k: _dev(v) for k, v in cloud.items()}
    for invert in (False, True):
        got, _ = _pc().select_by_mask(dev, _dev(mask), invert)
        _same_rows(got, orc.select_by_mask(cloud, mask, invert))


def test_select_reference_vectors():
    v = orc.reference_vectors()["select"]
    pts = orc.f32(v["points"])
    dev = {"positions": _dev(pts)}
    m = v["by_mask"]
    got, _ = _pc().select_by_mask(dev, _dev(np.array(m["mask"])))
    assert np.array_equal(got["positions"].cpu().numpy(),
                          orc.f32(m["expected"]))
    got, _ = _pc().select_by_mask(dev, _dev(np.array(m["mask"])), True)
    assert np.array_equal(got["positions"].cpu().numpy(),
                          orc.f32(m["expected_inverted"]))
    for case in v["by_index"]:
        got, _ = _pc().select_by_index(
            dev, _dev(np.array(case["indices"], np.int64)), case["invert"],
            case["remove_duplicates"])
        assert np.array_equal(got["positions"].cpu().numpy(),
                              orc.f32(case["expected"])), case


@pytest.mark.parametrize("invert,remove_duplicates",
                         [(False, False), (True, False), (False, True),
                          (True, True)])
def test_select_by_index_forms(invert, remove_duplicates):
    n = 3001
    cloud = _cloud(n, 3)
    idx = np.random.RandomState(4).randint(0, n, 2000).astype(np.int64)
    dev = {k: _dev(v) for k, v in cloud.items()}
    got, _ = _pc().select_by_index(dev, _dev(idx), invert, remove_duplicates)
    _same_rows(got, orc.select_by_index(cloud, idx, n, invert,
                                        remove_duplicates))


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("bad", [-1, 100])
def test_select_by_index_out_of_range_writes_nothing(bad, invert):
    from open3d_amd import _lib
    n = 100
    pts = _dev(np.random.RandomState(0).rand(n, 3).astype(np.float32))
    idx = _dev(np.array([3, 5, bad, 7], np.int64))
    out = torch.full((n, 3), -123.0, dtype=torch.float32, device="cuda")
    ins = (C.c_void_p * 1)(pts.data_ptr())
    outs = (C.c_void_p * 1)(out.data_ptr())
    widths = (C.c_int64 * 1)(12)
    m = C.c_int64(-7)
    st = _lib.lib().o3dmi_pointcloud_select_by_index(
        n, _lib.ptr(idx), 4, invert, 0, 1, ins, widths, outs, C.byref(m),
        None)
    torch.cuda.synchronize()
    assert st == INVALID_ARG
    assert bool((out == -123.0).all())


# ---- non-finite / duplicated -----------------------------------------------------------
def test_non_finite_reference_vectors():
    v = orc.reference_vectors()["non_finite_points"]
    pts = orc.f32(v["points"])
    for form in v["forms"]:
        got, mask = _pc().remove_non_finite_points(
            {"positions": _dev(pts)}, form["remove_nan"], form["remove_inf"])
        assert mask.cpu().numpy().tolist() == form["mask"], form
        if "expected" in form:
            assert np.array_equal(got["positions"].cpu().numpy(),
                                  orc.f32(form["expected"]))


def _awkward_points(dtype):
    """+-0, NaNs of equal and of unequal bits, infinities, 4096 copies of one
    point (the contended key), random points with duplicates."""
    rng = np.random.RandomState(21)
    base = rng.normal(size=(1500, 3)).astype(dtype)
    dup = base[rng.randint(0, 1500, 700)]
    zeros = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, 0.0], [0.0, -0.0, 0.0],
                      [0.0, 0.0, 0.0], [-0.0, 0.0, 0.0]], dtype)
    bits = np.uint32 if dtype == np.float32 else np.uint64
    qnan = np.array([np.nan], dtype).view(bits)[0]
    nan_a = np.array([qnan, qnan | bits(1), qnan], bits).view(dtype)
    nan_b = np.array([qnan, qnan | bits(2), qnan], bits).view(dtype)
    nans = np.stack([nan_a, nan_a, nan_b, nan_a, nan_b]).astype(dtype)
    assert nans.view(bits)[0, 1] != nans.view(bits)[2, 1]
    infs = np.array([[np.inf, 1, 2], [-np.inf, 1, 2], [np.inf, 1, 2],
                     [1, np.nan, np.inf]], dtype)
    hot = np.repeat(np.array([[0.5, -1.25, 3.0]], dtype), 4096, 0)
    p = np.concatenate([base, dup, zeros, nans, infs, hot])
    return np.ascontiguousarray(p[rng.permutation(p.shape[0])])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_non_finite_and_duplicated_masks(dtype):
    p = _awkward_points(dtype)
    dev = {"positions": _dev(p), "row": _dev(np.arange(p.shape[0]))}
    for rn, ri in ((True, True), (True, False), (False, True), (False, False)):
        got, mask = _pc().remove_non_finite_points(dev, rn, ri)
        want = orc.non_finite_mask(p, rn, ri)
        assert np.array_equal(mask.cpu().numpy(), want)
        assert np.array_equal(got["row"].cpu().numpy(), np.nonzero(want)[0])
    want = orc.duplicate_mask(p)
    for _ in range(2):  # the survivor is the lowest index on every run
        got, mask = _pc().remove_duplicated_points(dev)
        assert np.array_equal(mask.cpu().numpy(), want)
        assert np.array_equal(got["row"].cpu().numpy(), np.nonzero(want)[0])
        assert got["positions"].cpu().numpy().tobytes() == p[want].tobytes()


def test_duplicated_points_reference_vector():
    v = orc.reference_vectors()["duplicated_points"]
    got, _ = _pc().remove_duplicated_points(
        {"positions": _dev(orc.f32(v["points"]))})
    assert np.array_equal(got["positions"].cpu().numpy(),
                          orc.f32(v["expected"]))


# ---- radius ----------------------------------------------------------------------------
def test_radius_outliers_reference_vector():
    v = orc.reference_vectors()["radius_outliers"]
    got, _ = _pc().remove_radius_outliers(
        {"positions": _dev(orc.f32(v["points"]))}, v["nb_points"],
        v["search_radius"])
    assert np.array_equal(got["positions"].cpu().numpy(),
                          orc.f32(v["expected"]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_radius_outliers_mask_is_exact(dtype):
    p, pair = orc.radius_cloud(dtype)
    dev = {"positions": _dev(p)}
    for nb in orc.RADIUS_NB:
        got, mask = _pc().remove_radius_outliers(dev, nb, orc.RADIUS)
        want = orc.radius_mask(p, nb, orc.RADIUS)
        assert np.array_equal(mask.cpu().numpy(), want), nb
        assert got["positions"].cpu().numpy().tobytes() == p[want].tobytes()


# ---- statistical ---------------------------------------------------------------------------
def _close(got, want, rel=1e-12):
    # a float64 sum of N <= 4096 same-sign terms is within N * 2^-53 ~ 4.5e-13
    # of the exact sum in the worst order
    if np.isnan(want):
        return np.isnan(got)
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nb", orc.STAT_NB)
@pytest.mark.parametrize("size", orc.STAT_SIZES)
def test_statistical_outliers(size, nb, dtype):
    p = orc.stat_cloud(size, dtype)
    dev = {"positions": _dev(p), "row": _dev(np.arange(p.shape[0]))}
    for ratio in orc.STAT_RATIO:
        want = orc.stat_reference(size, dtype, nb, ratio)
        runs = []
        for _ in range(2):
            got, mask, stats = _pc().remove_statistical_outliers(
                dev, nb, ratio, return_stats=True)
            avg = stats["avg_distances"].cpu().numpy()
            runs.append((avg.tobytes(), mask.cpu().numpy().tobytes(),
                         np.array([stats["mean"], stats["std"],
                                   stats["threshold"]]).tobytes()))
        assert runs[0] == runs[1], "two runs differ"
        print("statistical %s nb=%d ratio=%g %s: mean %.17g (want %.17g) "
              "std %.17g (%.17g) threshold %.17g (%.17g) kept %d / %d" %
              (size, nb, ratio, np.dtype(dtype).name, stats["mean"],
               want["mean"], stats["std"], want["std"], stats["threshold"],
               want["threshold"], stats["kept"], p.shape[0]))
        assert avg.dtype == want["avg"].dtype
        assert avg.tobytes() == want["avg"].tobytes(), "avg_distances bits"
        assert _close(stats["mean"], want["mean"])
        assert _close(stats["std"], want["std"])
        assert _close(stats["threshold"], want["threshold"])
        assert np.array_equal(mask.cpu().numpy(), want["mask"])
        assert stats["kept"] == int(want["mask"].sum())
        assert np.array_equal(got["row"].cpu().numpy(),
                              np.nonzero(want["mask"])[0])


def _raw_statistical(points, nb, mask):
    from open3d_amd import _lib
    m = C.c_int64(-7)
    st = _lib.lib().o3dmi_pointcloud_remove_statistical_outliers(
        _lib.ptr(points), points.shape[0], _lib.F32, nb, C.c_double(2.0),
        _lib.ptr(mask), None, None, C.byref(m), None)
    torch.cuda.synchronize()
    return st


def test_statistical_outliers_limits_and_refusals():
    from open3d_amd import _lib
    p = orc.stat_cloud("n10", np.float32)
    mask = torch.full((10,), 77, dtype=torch.uint8, device="cuda")
    assert _raw_statistical(_dev(p), 65, mask) == UNSUPPORTED
    assert bool((mask == 77).all())
    p[4, 1] = np.nan
    assert _raw_statistical(_dev(p), 20, mask) == INVALID_ARG
    assert bool((mask == 77).all())
    p[4, 1] = np.inf
    m = C.c_int64(-7)
    st = _lib.lib().o3dmi_pointcloud_remove_radius_outliers(
        _lib.ptr(_dev(p)), 10, _lib.F32, 3, C.c_double(0.5), _lib.ptr(mask),
        C.byref(m), None)
    torch.cuda.synchronize()
    assert st == INVALID_ARG
    assert bool((mask == 77).all())


# ---- preprocess ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fragment():
    from open3d_amd import synthetic
    rng = np.random.RandomState(2)
    pair = synthetic.make_icp_pair(20000, 20000, seed=8)
    far = (rng.uniform(-1, 1, (40, 3)) * 2 + np.array([9.0, -8.0, 7.0]))
    p = np.concatenate([pair["target"], far.astype(np.float32)])
    nrm = np.concatenate([pair["target_normals"],
                          np.tile(np.float32([0, 0, 1]), (40, 1))])
    return _dev(p), _dev(nrm)


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("apply", [False, True])
def test_preprocess_equals_the_chain_of_public_calls(fragment, apply,
                                                     with_normals):
    from open3d_amd import registration, slac
    p, nrm = fragment
    nrm = nrm if with_normals else None
    got_p, got_n = slac.preprocess_point_cloud(p, nrm, 0.05, apply)
    dp, dn = registration.voxel_down_sample(p, nrm, 0.05)
    cloud = {"positions": dp}
    if dn is not None:
        cloud["normals"] = dn
    kept, mask = _pc().remove_statistical_outliers(cloud, 20, 2.0)
    assert 0 < int((~mask).sum()) < mask.shape[0] // 4
    if apply:
        cloud = kept
    want_n = registration.estimate_normals(cloud["positions"], 30, None,
                                           cloud.get("normals"))
    assert got_p.shape == cloud["positions"].shape
    assert torch.equal(got_p, cloud["positions"])
    assert got_n.cpu().numpy().tobytes() == want_n.cpu().numpy().tobytes()
    if not apply:
        # upstream's output: the filter is computed and dropped
        assert torch.equal(got_p, dp)


def test_preprocess_without_down_sampling(fragment):
    from open3d_amd import registration, slac
    p, nrm = fragment
    p, nrm = p[:6000].contiguous(), nrm[:6000].contiguous()
    # normals came in: they are kept, rows filtered only on request
    got_p, got_n = slac.preprocess_point_cloud(p, nrm, 0.0, False)
    assert torch.equal(got_p, p) and torch.equal(got_n, nrm)
    kept, mask = _pc().remove_statistical_outliers(
        {"positions": p, "normals": nrm}, 20, 2.0)
    got_p, got_n = slac.preprocess_point_cloud(p, nrm, 0.0, True)
    assert torch.equal(got_p, kept["positions"])
    assert torch.equal(got_n, kept["normals"])
    # none came in: estimated
    got_p, got_n = slac.preprocess_point_cloud(p, None, -1.0, False)
    want_n = registration.estimate_normals(p, 30, None)
    assert torch.equal(got_p, p)
    assert got_n.cpu().numpy().tobytes() == want_n.cpu().numpy().tobytes()
