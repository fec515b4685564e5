"""GPU tests of o3dmi_pointcloud_oriented_bounding_box (MINIMAL_APPROX, PCA),
o3dmi_pointcloud_oriented_bounding_ellipsoid and their Python mirrors against
the numpy oracle (tests/_bounding_volume_oracle.py). Every output is poisoned
before the call. The boxes are compared bit for bit; the ellipsoid by its
iteration count and within the tolerance measured in docs/bounding_volumes.md."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import _bounding_volume_oracle as orc
from test_bounding_volume_cpu import (gaussian_cloud, inside_box,
                                      inside_ellipsoid,
                                      scaled_sphere)

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, CAPACITY, SINGULAR, UNSUPPORTED = 0, 1, 3, 5, 7
APPROX, PCA, JYLANKI = 0, 1, 2
CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}
POISON = -777.0
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                    "open3d_amd", "csrc")

# The ellipsoid's tolerance (docs/bounding_volumes.md, "The measured
# tolerance"): the oracle run on the ellipsoid tests' clouds with its sums in
# the tree, in plain index order and in reverse order deviates by at most
# 2.75e-14 of the largest radius in centre, radii and ellipsoid points (the
# sphere of 4097 points; 3.2e-15 on the clouds of up to 500 points); 64 times
# that covers clouds not tried.
ELLIPSOID_TOL = 64 * 2.75e-14


def _constant(path, name):
    text = open(os.path.join(CSRC, path)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


assert "constexpr int kObbBlock = kBlock;" in open(
    os.path.join(CSRC, "bounding_volume.h")).read()
OBB_BLOCK = _constant("common.h", "kBlock")
OBB_TILE = _constant("bounding_volume.h", "kObbTile")
BV_BLOCK = _constant("bounding_volume.h", "kBvBlock")
BV_RUN = _constant("bounding_volume.h", "kBvRun")


def _L():
    from open3d_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _stream(stream):
    return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


class Result:
    def poisoned(self):
        return all((o == POISON).all() for o in self.outputs)


def _outputs():
    return [np.full(k, POISON) for k in (3, 9, 3)]


def _finish(r, st, outs):
    torch.cuda.synchronize()
    r.status, r.outputs = st, outs
    r.center, r.rotation, r.third = outs[0], outs[1].reshape(3, 3), outs[2]
    stats = (C.c_int64 * 5)()
    values = (C.c_double * 16)()
    assert _L().lib().o3dmi_internal_bounding_volume_stats(stats, values) == OK
    r.stats, r.values = list(stats), np.array(values)
    return r


def call_box(points, method=APPROX, stream=None, n=None, dtype=None,
             null=None, split=None):
    """One native call on poisoned outputs -> Result (third = extent). With
    split: the internal MINIMAL_APPROX call with that many vertex slices."""
    L = _L()
    points = np.ascontiguousarray(points)
    p = _dev(points)
    outs = _outputs()
    args = [L.ptr(p), len(points) if n is None else n,
            CODE[points.dtype] if dtype is None else dtype, method] + \
        [L.f64p(o) for o in outs] + [_stream(stream)]
    if null is not None:
        args[null] = None
    if split is not None:
        args[3] = split
        return _finish(
            Result(),
            L.lib().o3dmi_internal_pointcloud_obb_minimal_approx(*args), outs)
    return _finish(Result(), L.lib().o3dmi_pointcloud_oriented_bounding_box(
        *args), outs)


def call_ellipsoid(points, stream=None, n=None, dtype=None, null=None,
                   iterations=True):
    """One native call on poisoned outputs -> Result (third = radii)."""
    L = _L()
    points = np.ascontiguousarray(points)
    p = _dev(points)
    outs = _outputs()
    it = C.c_int32(int(POISON))
    args = [L.ptr(p), len(points) if n is None else n,
            CODE[points.dtype] if dtype is None else dtype] + \
        [L.f64p(o) for o in outs] + [C.byref(it) if iterations else None,
                                     _stream(stream)]
    if null is not None:
        args[null] = None
    r = _finish(Result(),
                L.lib().o3dmi_pointcloud_oriented_bounding_ellipsoid(*args),
                outs)
    r.iterations = it.value
    return r


# ---- the clouds and their oracles, computed once ------------------------------------
# hull sizes at the edges: a tetrahedron, 5, the wave +- 1, the workgroup of
# (a) +- 1, one past its vertex tile; on the scaled sphere V = n
EDGE_SIZES = [4, 5, 64, 65, OBB_BLOCK - 1, OBB_BLOCK, OBB_BLOCK + 1,
              OBB_TILE + 1]


def cloud(name):
    kind, _, arg = name.partition(":")
    dtype = np.float32 if name.endswith("f32") else np.float64
    if kind == "gaussian":
        return gaussian_cloud(dtype)
    return scaled_sphere(int(arg.split("/")[0]), dtype=dtype)


CLOUDS = ["gaussian", "gaussian:/f32"] + \
    ["sphere:%d" % n for n in EDGE_SIZES] + ["sphere:%d/f32" % (OBB_BLOCK + 1)]


@functools.lru_cache(maxsize=None)
def oracle(name):
    points = cloud(name)
    X, tri, idx = orc.hull_of(points)
    if name.startswith("sphere"):
        assert len(X) == len(points)
    return X, tri


@functools.lru_cache(maxsize=None)
def oracle_ellipsoid(name):
    return orc.ellipsoid(oracle(name)[0])


# ---- (a) bit for bit ----------------------------------------------------------------
def expect_box(r, want):
    assert r.status == OK
    assert _same_bits(r.center, want["center"])
    assert _same_bits(r.rotation, want["rotation"])
    assert _same_bits(r.third, want["extent"])
    assert _same_bits(r.values[9:12], want["lo"])
    assert _same_bits(r.values[12:15], want["hi"])


@pytest.mark.parametrize("name", CLOUDS)
def test_minimal_approx_bits(name):
    X, tri = oracle(name)
    want = orc.minimal_approx(X, tri)
    v = np.sort(want["volumes"][~np.isnan(want["volumes"])])
    assert v[1] >= v[0] * (1.0 + 1e-6), "the winner is not unique"
    r = call_box(cloud(name), APPROX)
    assert r.stats[:2] == [len(X), len(tri)]
    assert r.stats[4] == want["winner"]
    expect_box(r, want)


@pytest.mark.parametrize("split", [2, 3, 64])
def test_minimal_approx_split_over_vertices_gives_the_same_bits(split):
    name = "sphere:%d" % (OBB_TILE + 1)
    X, tri = oracle(name)
    r = call_box(cloud(name), split=split)
    want = orc.minimal_approx(X, tri)
    assert r.stats[4] == want["winner"]
    expect_box(r, want)


# ---- (b) bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("name", CLOUDS)
def test_pca_bits(name):
    X, tri = oracle(name)
    want = orc.pca(X)
    r = call_box(cloud(name), PCA)
    assert r.stats[:2] == [len(X), len(tri)]
    assert _same_bits(r.values[:9], want["sums"])
    expect_box(r, want)


def test_pca_sums_over_several_workgroups():
    """V above one workgroup's slice of the tree: the partial rows and the
    last arrival. Every point of the scaled sphere is a vertex, so the oracle
    needs no hull."""
    n = BV_BLOCK * BV_RUN + 1
    pts = scaled_sphere(n, seed=9)
    r = call_box(pts, PCA)
    assert r.stats[0] == n
    want = orc.pca(pts)
    assert _same_bits(r.values[:9], want["sums"])
    expect_box(r, want)


# ---- (c) against the oracle ---------------------------------------------------------
def ellipsoid_points(center, R, radii):
    ax = (R * radii[None, :]).T
    return np.array([center + s * ax[k] for k in range(3) for s in (1, -1)])


def expect_ellipsoid(r, want):
    assert r.status == OK
    assert r.iterations == want["iterations"] == r.stats[2]
    scale = float(want["radii"].max())
    tol = ELLIPSOID_TOL * scale
    for got, ref in ((r.center, want["center"]), (r.third, want["radii"]),
                     (ellipsoid_points(r.center, r.rotation, r.third),
                      ellipsoid_points(want["center"], want["rotation"],
                                       want["radii"]))):
        print("deviation / largest radius:", np.abs(got - ref).max() / scale)
        assert np.abs(got - ref).max() <= tol


@pytest.mark.parametrize("name", ["gaussian", "gaussian:/f32", "sphere:500",
                                  "sphere:4", "sphere:65"])
def test_ellipsoid_against_the_oracle(name):
    want = oracle_ellipsoid(name)
    if name.startswith("gaussian"):
        assert want["iterations"] == orc.MAX_ITERATIONS
    if name == "sphere:500":
        assert 1 < want["iterations"] < orc.MAX_ITERATIONS
    r = call_ellipsoid(cloud(name))
    assert r.stats[3] == 0  # resident
    expect_ellipsoid(r, want)


@pytest.mark.parametrize("name", ["gaussian", "sphere:500"])
def test_ellipsoid_streamed_form_gives_the_resident_bits(name, monkeypatch):
    a = call_ellipsoid(cloud(name))
    monkeypatch.setenv("O3DMI_OBE_FORM", "streamed")
    b = call_ellipsoid(cloud(name))
    assert (a.stats[3], b.stats[3]) == (0, 1)
    assert a.status == b.status == OK and a.iterations == b.iterations
    for x, y in zip(a.outputs, b.outputs):
        assert _same_bits(x, y)
    assert _same_bits(a.values, b.values)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_ellipsoid_forms_at_the_capacity(delta, monkeypatch):
    cap = _L().lib().o3dmi_internal_obe_resident_capacity()
    assert cap == BV_BLOCK * BV_RUN
    n = cap + delta
    pts = scaled_sphere(n, seed=10)
    want = orc.ellipsoid(pts)  # V = n: every point is a vertex
    monkeypatch.setenv("O3DMI_OBE_FORM", "streamed")
    s = call_ellipsoid(pts)
    assert s.stats[0] == n and s.stats[3] == 1
    expect_ellipsoid(s, want)
    monkeypatch.setenv("O3DMI_OBE_FORM", "resident")
    r = call_ellipsoid(pts)
    if delta > 0:
        assert r.status == CAPACITY and r.poisoned()
        monkeypatch.delenv("O3DMI_OBE_FORM")
        assert call_ellipsoid(pts).stats[3] == 1
        return
    assert r.stats[3] == 0 and r.iterations == s.iterations
    for x, y in zip(r.outputs, s.outputs):
        assert _same_bits(x, y)


# ---- properties on symmetric inputs -------------------------------------------------
LATTICE = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"),
                   -1).reshape(-1, 3)
CORNERS = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-2.0, 2.0)
                    for z in (-3.0, 3.0)])


def unit_sphere():
    g = np.random.default_rng(31).standard_normal((300, 3))
    return g / np.linalg.norm(g, axis=1, keepdims=True)


SYMMETRIC = {"lattice": LATTICE, "corners": CORNERS, "sphere": unit_sphere()}


def _rotation_ok(R, proper):
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
    det = np.linalg.det(R)
    assert abs((det if proper else abs(det)) - 1.0) <= 1e-12


@pytest.mark.parametrize("method", [APPROX, PCA])
@pytest.mark.parametrize("name", sorted(SYMMETRIC))
def test_box_properties_on_symmetric_inputs(name, method):
    pts = SYMMETRIC[name]
    r = call_box(pts, method)
    assert r.status == OK
    assert inside_box(pts, r.center, r.rotation, r.third, orc.slack(pts))
    _rotation_ok(r.rotation, proper=True)
    if method == APPROX:
        # candidate -1 is the axis-aligned box (PCA has no such candidate: on
        # a degenerate covariance its frame is any rotation)
        aabb = pts.max(axis=0) - pts.min(axis=0)
        e = r.third
        assert (e[0] * e[1]) * e[2] <= (aabb[0] * aabb[1]) * aabb[2]


@pytest.mark.parametrize("name", sorted(SYMMETRIC))
def test_ellipsoid_properties_on_symmetric_inputs(name):
    """max M is the one at the weights the loop ends with (see
    test_bounding_volume_cpu.inside_ellipsoid); upstream's closest-identity
    step picks among all 48 signed permutations, so its rotation is orthonormal
    with det +1 or -1."""
    pts = SYMMETRIC[name]
    r = call_ellipsoid(pts)
    assert r.status == OK
    X, _, _ = orc.hull_of(pts)
    want = orc.ellipsoid(X)
    assert r.iterations == want["iterations"]
    _rotation_ok(r.rotation, proper=False)
    Q = r.rotation @ np.diag(1.0 / (r.third * r.third)) @ r.rotation.T
    assert inside_ellipsoid(pts, r.center, Q, want["final_max_m"],
                            orc.slack(pts))
    if name != "sphere":  # one iteration with step ~ 0: the last M bounds too
        assert inside_ellipsoid(pts, r.center, Q, want["max_m"],
                                orc.slack(pts))


# ---- protocol -----------------------------------------------------------------------
def test_refusals_leave_the_outputs_poisoned():
    good = gaussian_cloud()
    nan = good.copy()
    nan[17, 1] = np.nan
    inf = good.astype(np.float32)
    inf[299, 2] = np.inf
    for r in (call_box(good, n=3), call_box(good, n=2 ** 31 - 1),
              call_box(good, null=0), call_box(good, dtype=4),
              call_box(good, method=3), call_box(good, method=-1),
              call_box(good, null=4), call_box(good, null=5),
              call_box(good, null=6), call_box(nan), call_box(inf, PCA),
              call_box(good, split=0), call_box(good, split=65),
              call_ellipsoid(good, n=3), call_ellipsoid(good, n=2 ** 31 - 1),
              call_ellipsoid(good, null=0), call_ellipsoid(good, dtype=5),
              call_ellipsoid(good, null=3), call_ellipsoid(good, null=4),
              call_ellipsoid(good, null=5), call_ellipsoid(nan),
              call_ellipsoid(inf)):
        assert r.status == INVALID_ARG and r.poisoned()
    r = call_box(good, JYLANKI)
    assert r.status == UNSUPPORTED and r.poisoned()
    flat = good.copy()
    flat[:, 2] = 1.5
    for r in (call_box(flat), call_box(flat, PCA), call_ellipsoid(flat)):
        assert r.status == SINGULAR and r.poisoned()
    assert call_ellipsoid(good, iterations=False).status == OK


def test_repeated_cloud_and_repeated_calls_give_the_same_bits():
    pts = gaussian_cloud()
    twice = np.concatenate([pts, pts])
    for call in (lambda p: call_box(p, APPROX), lambda p: call_box(p, PCA),
                 call_ellipsoid):
        first = call(pts)
        assert first.status == OK
        for other in (call(pts), call(pts), call(twice)):
            assert other.status == OK
            for x, y in zip(first.outputs, other.outputs):
                assert _same_bits(x, y)


def test_non_default_stream():
    pts = gaussian_cloud()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for call in (lambda p, s: call_box(p, APPROX, s),
                     lambda p, s: call_box(p, PCA, s), call_ellipsoid):
            a, b = call(pts, None), call(pts, stream)
            assert a.status == b.status == OK
            for x, y in zip(a.outputs, b.outputs):
                assert _same_bits(x, y)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_python_mirror(dtype):
    from open3d_amd import pointcloud, trianglemesh
    pts = gaussian_cloud(dtype)
    p = _dev(pts)
    X, tri, _ = orc.hull_of(pts)
    t = p.dtype
    for method, want in (("minimal_approx", orc.minimal_approx(X, tri)),
                         ("pca", orc.pca(X))):
        box = pointcloud.get_oriented_bounding_box({"positions": p},
                                                   method=method)
        mesh_box = trianglemesh.get_oriented_bounding_box(
            {"positions": p}, method=method)
        for key, shape in (("center", (3,)), ("rotation", (3, 3)),
                           ("extent", (3,))):
            assert box[key].dtype == t and box[key].device == p.device
            assert tuple(box[key].shape) == shape
            assert torch.equal(box[key], mesh_box[key])
            assert torch.equal(box[key].cpu(), torch.from_numpy(
                np.ascontiguousarray(want[key])).to(t))
        corners = pointcloud.box_points(box)
        assert corners.dtype == t and tuple(corners.shape) == (8, 3)
        ref = orc.box_points(*(box[k].cpu().double().numpy()
                               for k in ("center", "rotation", "extent")))
        assert np.allclose(corners.cpu().double().numpy(), ref, rtol=0,
                           atol=1e-5 if dtype == np.float32 else 1e-13)
    e = pointcloud.get_oriented_bounding_ellipsoid({"positions": p})
    m = trianglemesh.get_oriented_bounding_ellipsoid({"positions": p})
    for key in ("center", "rotation", "radii"):
        assert e[key].dtype == t and e[key].device == p.device
        assert torch.equal(e[key], m[key])
    six = pointcloud.ellipsoid_points(e)
    assert six.dtype == t and tuple(six.shape) == (6, 3)
    ref = ellipsoid_points(*(e[k].cpu().double().numpy()
                             for k in ("center", "rotation", "radii")))
    assert np.allclose(six.cpu().double().numpy(), ref, rtol=0,
                       atol=1e-5 if dtype == np.float32 else 1e-13)
    with pytest.raises(_L().O3DMIError) as err:
        pointcloud.get_oriented_bounding_box({"positions": p},
                                             method="minimal_jylanki")
    assert err.value.status == UNSUPPORTED


@pytest.mark.parametrize("method", ["minimal_approx", "pca"])
def test_crop_with_the_returned_box_keeps_every_point(method):
    from open3d_amd import pointcloud
    pts = gaussian_cloud()
    cloud_ = {"positions": _dev(pts)}
    box = pointcloud.get_oriented_bounding_box(cloud_, method=method)
    inflated = box["extent"] + 2.0 * orc.slack(pts)
    kept = pointcloud.crop(cloud_, center=box["center"],
                           rotation=box["rotation"], extent=inflated)
    assert kept["positions"].shape[0] == len(pts)
    assert torch.equal(kept["positions"], cloud_["positions"])
