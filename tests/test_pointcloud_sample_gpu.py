"""GPU tests of PointCloud::FarthestPointDownSample, UniformDownSample,
RandomDownSample, Crop and the bounds against the numpy oracle
(tests/_pointcloud_sample_oracle.py). Everything is compared bit for bit:
the feature has no tolerance.

The farthest-point order runs in both kernel forms (1 = resident, 2 =
streamed); each is held against the oracle and against the other. The streamed
form never runs more than 256 samples here (one launch each)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _pointcloud_sample_oracle as orc

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, 7
F32, F64 = 0, 1
DTYPES = [np.float32, np.float64]
CODE = {np.float32: F32, np.float64: F64}


def _pc():
    from open3d_amd import pointcloud
    return pointcloud


def _L():
    from open3d_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- farthest point: the clouds ------------------------------------------------
def _golden(name):
    for case in orc.reference_vectors()["farthest_point"]:
        if case["name"] == name:
            return case
    raise KeyError(name)


def _lattice():
    g = np.arange(12, dtype=np.float64) * 0.01
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def _overflow():
    # squares of the large differences overflow Float32: ties at +inf
    rng = np.random.RandomState(5)
    return rng.choice([-3e19, -2.9e19, 2.9e19, 3e19], size=(200, 3))


def _random(n, seed):
    return np.random.RandomState(seed).standard_normal((n, 3))


# name -> (points float64, num_samples, start_index)
@functools.lru_cache(maxsize=None)
def _clouds():
    out = {}
    for name in ("upstream_start0", "upstream_start4", "duplicates"):
        c = _golden(name)
        out[name] = (np.array(c["points"], np.float64), c["num_samples"],
                     c["start_index"])
    out["n1"] = (_random(1, 1), 1, 0)
    for n in (63, 64, 65, 1023, 1024, 1025):   # wave and workgroup edges
        out["n%d" % n] = (_random(n, n), min(n, 48), n // 3)
    out["start_last"] = (_random(777, 3), 40, 776)
    out["lattice"] = (_lattice(), 64, 0)        # many exact ties
    out["overflow"] = (_overflow(), 32, 7)
    # streamed form: three workgroups, the last one partly filled; and one
    # point more than two whole slices
    out["blocks_700"] = (_random(700, 11), 32, 5)
    out["blocks_513"] = (_random(513, 12), 32, 512)
    return out


CLOUDS = ["upstream_start0", "upstream_start4", "duplicates", "n1", "n63",
          "n64", "n65", "n1023", "n1024", "n1025", "start_last", "lattice",
          "overflow", "blocks_700", "blocks_513"]


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    pts, k, start = _clouds()[name]
    pts = pts.astype(dtype)
    want = orc.farthest_point_order(pts, k, start)
    want.setflags(write=False)
    return pts, k, start, want


# the squares of "overflow" only overflow in Float32
ORDER_CASES = [(name, dtype) for name in CLOUDS for dtype in DTYPES
               if (name, dtype) != ("overflow", np.float64)]


@pytest.mark.parametrize("name,dtype", ORDER_CASES)
def test_farthest_point_order_both_forms(name, dtype):
    pts, k, start, want = _case(name, dtype)
    p = _dev(pts)
    got = {form: _pc().farthest_point_order(p, k, start, form).cpu().numpy()
           for form in (1, 2, 0)}
    print(name, dtype.__name__, "oracle", want[:8], "resident", got[1][:8],
          "streamed", got[2][:8])
    assert np.array_equal(got[1], want)
    assert np.array_equal(got[2], want)
    assert np.array_equal(got[1], got[2])
    assert np.array_equal(got[0], want)


def test_the_clouds_test_what_they_claim():
    _, k, _, want = _case("lattice", np.float32)
    assert len(set(want.tolist())) == k == 64
    assert _case("duplicates", np.float64)[3].tolist() == [0, 3, 0, 0]
    pts, k, start, want = _case("overflow", np.float32)
    with np.errstate(over="ignore"):
        d = ((pts - pts[start]) ** 2).sum(axis=1)
    assert np.isinf(d).sum() > 1 and np.isfinite(d).sum() > 1
    assert _case("start_last", np.float32)[2] == 776


@pytest.mark.parametrize("dtype", DTYPES)
def test_streamed_form_with_slices_above_one_stride(dtype):
    """262145 points: slices of 512, 513 workgroups, one point in the last."""
    n, k = 262145, 8
    pts = _random(n, 21).astype(dtype)
    want = orc.farthest_point_order(pts, k, 9)
    got = _pc().farthest_point_order(_dev(pts), k, 9, 2).cpu().numpy()
    assert np.array_equal(got, want)
    assert _L().lib().o3dmi_pointcloud_farthest_point_order(
        _L().ptr(_dev(pts)), n, CODE[dtype], k, 9, 1,
        _L().ptr(torch.empty(k, dtype=torch.int64, device="cuda")),
        None) == UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES)
def test_form_by_size_at_the_capacity(dtype):
    cap = _L().lib().o3dmi_pointcloud_farthest_point_capacity(CODE[dtype])
    assert cap >= 1024
    pts = _random(cap + 1, 31).astype(dtype)
    for n in (cap, cap + 1):
        want = orc.farthest_point_order(pts[:n], 32, n - 1)
        p = _dev(pts[:n])
        got = _pc().farthest_point_order(p, 32, n - 1, 0).cpu().numpy()
        assert np.array_equal(got, want), n
    # at the capacity both forms run, and agree
    p = _dev(pts[:cap])
    a = _pc().farthest_point_order(p, 32, 0, 1)
    b = _pc().farthest_point_order(p, 32, 0, 2)
    assert torch.equal(a, b)


def test_two_calls_give_the_same_bits():
    pts, k, start, _ = _case("n1025", np.float32)
    p = _dev(pts)
    for form in (1, 2):
        a = _pc().farthest_point_order(p, k, start, form)
        b = _pc().farthest_point_order(p, k, start, form)
        assert torch.equal(a, b)


# ---- farthest point: the mask call ---------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["upstream_start0", "upstream_start4",
                                  "duplicates", "n1025"])
def test_farthest_point_mask_is_the_set_of_the_order(name, dtype):
    pts, k, start, want = _case(name, dtype)
    mask, kept, order = _pc().farthest_point_mask(_dev(pts), k, start,
                                                  return_order=True)
    want_mask = orc.farthest_point_mask(pts, k, start)
    assert np.array_equal(order.cpu().numpy(), want)
    assert np.array_equal(mask.cpu().numpy().astype(bool), want_mask)
    assert kept == want_mask.sum() == len(set(want.tolist()))
    if name == "duplicates":
        assert kept == 2
    # the mirror: rows in input order, every attribute carried through
    attrs = {"positions": _dev(pts),
             "colors": _dev(np.arange(3 * len(pts), dtype=np.uint8)
                            .reshape(-1, 3))}
    out = _pc().farthest_point_down_sample(attrs, k, start)
    assert np.array_equal(out["positions"].cpu().numpy(), pts[want_mask])
    assert torch.equal(out["colors"].cpu(), attrs["colors"].cpu()[want_mask])
    if name != "n1025":
        assert np.flatnonzero(want_mask).tolist() == \
            _golden(name)["expected_indices"]


def test_farthest_point_mask_shortcuts_and_refusals():
    pts, _, _, _ = _case("n65", np.float32)
    n = len(pts)
    p = _dev(pts)
    mask, kept = _pc().farthest_point_mask(p, 0)
    assert kept == 0 and not mask.any()
    mask, kept = _pc().farthest_point_mask(p, n, 3)
    assert kept == n and bool((mask == 1).all())
    # num_samples == n with an order: the loop still runs
    mask, kept, order = _pc().farthest_point_mask(p, n, 3, return_order=True)
    assert kept == n and bool((mask == 1).all())
    assert np.array_equal(order.cpu().numpy(),
                          orc.farthest_point_order(pts, n, 3))
    # a NaN coordinate is refused, the outputs untouched
    L = _L()
    for bad_value in (np.nan, np.inf):
        bad = pts.copy()
        bad[40, 1] = bad_value
        b = _dev(bad)
        mask = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        order = torch.full((4,), -9, dtype=torch.int64, device="cuda")
        m = C.c_int64(-5)
        st = L.lib().o3dmi_pointcloud_farthest_point_down_sample(
            L.ptr(b), n, F32, 4, 0, L.ptr(mask), None, C.byref(m), None)
        assert st == INVALID_ARG and m.value == -5
        assert bool((mask == 7).all())
        for form in (0, 1, 2):
            st = L.lib().o3dmi_pointcloud_farthest_point_order(
                L.ptr(b), n, F32, 4, 0, form, L.ptr(order), None)
            assert st == INVALID_ARG and bool((order == -9).all())


# ---- uniform ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 8, 100])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9])
def test_uniform_down_sample(n, k):
    rng = np.random.RandomState(100 * n + k)
    attrs = {"positions": rng.standard_normal((n, 3)).astype(np.float32),
             "colors": rng.randint(0, 256, (n, 3)).astype(np.uint8),
             "normals64": rng.standard_normal((n, 3))}
    assert [3 * a.dtype.itemsize for a in attrs.values()] == [12, 3, 24]
    out = _pc().uniform_down_sample({k_: _dev(a) for k_, a in attrs.items()},
                                    k)
    for name, a in attrs.items():
        assert np.array_equal(out[name].cpu().numpy(), a[::k]), name
        assert out[name].shape[0] == (n + k - 1) // k


def test_uniform_golden():
    v = orc.reference_vectors()["uniform"]
    pts = np.array(v["points"], np.float32)
    out = _pc().uniform_down_sample({"positions": _dev(pts)},
                                    v["every_k_points"])
    assert np.array_equal(out["positions"].cpu().numpy(),
                          pts[v["expected_rows"]])


# ---- random -----------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 1000])
def test_random_down_sample(n, ratio):
    seed = 0xC0FFEE + n
    want = orc.random_sample_indices(n, ratio, seed)
    got = _pc().random_sample_indices(n, ratio, seed).cpu().numpy()
    assert len(got) == int(ratio * n)
    assert np.array_equal(got, want)
    assert len(set(got.tolist())) == len(got)
    assert got.size == 0 or (got.min() >= 0 and got.max() < n)
    rng = np.random.RandomState(n)
    attrs = {"positions": rng.standard_normal((n, 3)),
             "colors": rng.randint(0, 256, (n, 3)).astype(np.uint8)}
    out = _pc().random_down_sample({k: _dev(a) for k, a in attrs.items()},
                                   ratio, seed)
    for name, a in attrs.items():
        assert np.array_equal(out[name].cpu().numpy(), a[want]), name
    if len(want) > 8:
        other = _pc().random_sample_indices(n, ratio, seed + 1).cpu().numpy()
        assert not np.array_equal(other, want)


# ---- crop -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_crop_goldens(dtype):
    v = orc.reference_vectors()
    for case in v["aabb"]:
        pts = np.array(case["points"], dtype)
        out = _pc().crop({"positions": _dev(pts)}, min_bound=case["min_bound"],
                         max_bound=case["max_bound"])
        assert np.array_equal(out["positions"].cpu().numpy(),
                              pts[case["expected_indices"]])
    for case in v["obb"]:
        pts = np.array(case["points"], dtype)
        out = _pc().crop({"positions": _dev(pts)}, center=case["center"],
                         rotation=case["rotation"], extent=case["extent"])
        assert np.array_equal(out["positions"].cpu().numpy(),
                              pts[case["expected_indices"]]), case["name"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_crop_faces_nan_rows_and_invert(dtype):
    # centred on the origin, so that the oriented form's p - center is exact
    lo, hi = [-1.0, -0.5, -4.0], [1.0, 0.5, 4.0]
    mid = [0.0, 0.0, 0.0]
    rows = [mid]
    for axis in range(3):
        for bound, step in ((lo, -1), (hi, 1)):
            on = list(mid)
            on[axis] = bound[axis]
            rows.append(on)                      # exactly on the face: inside
            off = np.array(on, dtype)
            off[axis] = np.nextafter(off[axis], dtype(step * np.inf))
            rows.append(off.tolist())            # one ulp beyond: outside
    rows.append([np.nan, 0.0, 0.0])              # fails every comparison
    rows.append([0.0, 0.0, np.nan])
    pts = np.array(rows, dtype)
    want = orc.aabb_mask(pts, lo, hi)
    assert want.tolist() == [True] + [True, False] * 6 + [False, False]
    attrs = {"positions": _dev(pts),
             "ids": _dev(np.arange(len(pts), dtype=np.int32))}
    out = _pc().crop(attrs, min_bound=lo, max_bound=hi)
    assert out["ids"].cpu().numpy().tolist() == np.flatnonzero(want).tolist()
    out = _pc().crop(attrs, min_bound=lo, max_bound=hi, invert=True)
    assert out["ids"].cpu().numpy().tolist() == np.flatnonzero(~want).tolist()
    # the same box as an oriented one (identity rotation): same rows
    center = [(a + b) / 2 for a, b in zip(lo, hi)]
    extent = [b - a for a, b in zip(lo, hi)]
    want_obb = orc.obb_mask(pts, center, np.eye(3), extent)
    assert want_obb.tolist() == want.tolist()
    out = _pc().crop(attrs, center=center, rotation=np.eye(3), extent=extent)
    assert out["ids"].cpu().numpy().tolist() == \
        np.flatnonzero(want_obb).tolist()
    out = _pc().crop(attrs, center=center, rotation=np.eye(3), extent=extent,
                     invert=True)
    assert out["ids"].cpu().numpy().tolist() == \
        np.flatnonzero(~want_obb).tolist()


def test_crop_random_rotated_box_equals_the_oracle():
    rng = np.random.RandomState(8)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    for dtype in DTYPES:
        pts = rng.standard_normal((1000, 3)).astype(dtype)
        want = orc.obb_mask(pts, [0.1, -0.2, 0.3], q, [1.5, 1.0, 2.0])
        assert 50 < want.sum() < 950
        mask = torch.empty(1000, dtype=torch.uint8, device="cuda")
        m = C.c_int64(0)
        L = _L()
        v = lambda x: (C.c_double * len(x))(*x)
        assert L.lib().o3dmi_pointcloud_obb_mask(
            L.ptr(_dev(pts)), 1000, CODE[dtype], v([0.1, -0.2, 0.3]),
            v(q.reshape(-1).tolist()), v([1.5, 1.0, 2.0]), L.ptr(mask),
            C.byref(m), None) == 0
        assert np.array_equal(mask.cpu().numpy().astype(bool), want)
        assert m.value == want.sum()


def test_crop_empty_box_through_the_mirror():
    pts = _random(20, 2).astype(np.float32)
    attrs = {"positions": _dev(pts)}
    flat = dict(min_bound=[-9, -9, 0.5], max_bound=[9, 9, 0.5])
    assert _pc().crop(attrs, **flat)["positions"].shape == (0, 3)
    out = _pc().crop(attrs, invert=True, **flat)
    assert np.array_equal(out["positions"].cpu().numpy(), pts)
    flat = dict(center=[0, 0, 0], rotation=np.eye(3), extent=[9, 0, 9])
    assert _pc().crop(attrs, **flat)["positions"].shape == (0, 3)
    out = _pc().crop(attrs, invert=True, **flat)
    assert np.array_equal(out["positions"].cpu().numpy(), pts)
    with pytest.raises(ValueError):
        _pc().crop(attrs, min_bound=[0, 0, 0], max_bound=[1, -1, 1])
    with pytest.raises(ValueError):
        _pc().crop(attrs, min_bound=[0, 0, 0])


def test_crop_bounds_are_rounded_to_the_point_dtype():
    """0.1 as a double lies below float32(0.1); rounded to Float32 it equals
    the coordinate, so the point on that face is inside, as upstream's
    .To(dtype) has it."""
    x = np.float32(0.1)
    assert float(x) > 0.1
    pts = np.array([[x, 0, 0], [-x, 0, 0]], np.float32)
    attrs = {"positions": _dev(pts)}
    out = _pc().crop(attrs, min_bound=[-0.1, -1, -1], max_bound=[0.1, 1, 1])
    assert out["positions"].shape[0] == 2
    # in Float64 the same numbers are outside
    out = _pc().crop({"positions": _dev(pts.astype(np.float64))},
                     min_bound=[-0.1, -1, -1], max_bound=[0.1, 1, 1])
    assert out["positions"].shape[0] == 0
    out = _pc().crop(attrs, center=[0, 0, 0], rotation=np.eye(3),
                     extent=[0.2, 2, 2])
    assert out["positions"].shape[0] == 2


# ---- bounds -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 65, 100003])
def test_min_max_bound(n, dtype):
    pts = (_random(n, n) * 100).astype(dtype)
    attrs = {"positions": _dev(pts)}
    lo, hi = _pc().get_min_bound(attrs), _pc().get_max_bound(attrs)
    assert lo.dtype == torch.float64
    assert np.array_equal(lo.numpy(), pts.min(axis=0).astype(np.float64))
    assert np.array_equal(hi.numpy(), pts.max(axis=0).astype(np.float64))


def test_min_max_bound_of_an_empty_cloud_is_zero():
    attrs = {"positions": torch.empty((0, 3), dtype=torch.float32,
                                      device="cuda")}
    assert _pc().get_min_bound(attrs).tolist() == [0, 0, 0]
    assert _pc().get_max_bound(attrs).tolist() == [0, 0, 0]
