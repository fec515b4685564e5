"""GPU tests of o3dmi_pointcloud_convex_hull / o3dmi_pointcloud_hidden_point_
removal and their Python mirrors against the goldens recorded from Qhull and
the numpy oracle (tests/_pointcloud_hull_oracle.py). Every output is poisoned
before the call; every comparison is bit for bit."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import _pointcloud_hull_oracle as orc
from test_pointcloud_hull_cpu import GOLDENS, golden, refusal_cases, six_volume

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, CAPACITY, SINGULAR = 0, 1, 3, 5
CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1,
        np.dtype(np.int32): 4, np.dtype(np.int64): 5}
POISON = -777
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                    "open3d_amd", "csrc")


def _constant(path, name):
    text = open(os.path.join(CSRC, path)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


# the workgroup of the hull kernels (pointcloud_hull.h: kHullBlock = kBlock),
# the tile of the prefix sums they feed (scan.hip) and the walk's list
assert "constexpr int kHullBlock = kBlock;" in open(
    os.path.join(CSRC, "pointcloud_hull.h")).read()
HULL_BLOCK = _constant("common.h", "kBlock")
SCAN_TILE = _constant("scan.hip", "kScanBlock") * \
    _constant("scan.hip", "kScanItems")
WALK_CAP = _constant("pointcloud_hull.h", "kHullWalkCap")


def _L():
    from open3d_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poison(shape, np_dtype):
    dtype = torch.from_numpy(np.zeros(0, np_dtype)).dtype
    return torch.full(shape, POISON, dtype=dtype, device="cuda")


def _poisoned(t):
    return bool((t == POISON).all())


class Result:
    pass


def call_abi(points, index=np.int32, hpr=None, vcap=None, tcap=None):
    """One native call on poisoned outputs -> Result(status, nv, nt, pos, idx,
    tri as numpy, whole buffers)."""
    L = _L()
    points = np.ascontiguousarray(points)
    n = len(points)
    p = _dev(points) if n else None
    vcap = n if vcap is None else vcap
    tcap = max(2 * n - 4, 0) if tcap is None else tcap
    pos = _poison((max(vcap, 0), 3), points.dtype)
    idx = _poison((max(vcap, 0),), index)
    tri = _poison((max(tcap, 0), 3), index)
    nv, nt = C.c_int64(-5), C.c_int64(-5)
    out = (L.ptr(pos), L.ptr(idx), vcap, L.ptr(tri), tcap,
           CODE[np.dtype(index)], C.byref(nv), C.byref(nt),
           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    head = (L.ptr(p) if n else C.c_void_p(8), n, CODE[points.dtype])
    if hpr is None:
        st = L.lib().o3dmi_pointcloud_convex_hull(*head, *out)
    else:
        cam = (C.c_double * 3)(*[float(e) for e in hpr[0]])
        st = L.lib().o3dmi_pointcloud_hidden_point_removal(
            *head, cam, C.c_double(hpr[1]), *out)
    torch.cuda.synchronize()
    r = Result()
    r.status, r.nv, r.nt = st, nv.value, nt.value
    r.pos, r.idx, r.tri = pos.cpu().numpy(), idx.cpu().numpy(), \
        tri.cpu().numpy()
    return r


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def expect(r, points, want_idx, want_tri, index=np.int32):
    """The result equals (want_idx, want_tri): counts, bit copies of the named
    rows, indices, triangles, and poison behind the counts."""
    assert r.status == OK
    assert (r.nv, r.nt) == (len(want_idx), len(want_tri))
    assert r.idx.dtype == np.dtype(index) and r.tri.dtype == np.dtype(index)
    assert np.array_equal(r.idx[:r.nv], want_idx)
    assert np.array_equal(r.tri[:r.nt], want_tri)
    assert r.pos.dtype == points.dtype
    assert np.array_equal(_bits(r.pos[:r.nv]), _bits(points[want_idx]))
    assert (r.pos[r.nv:] == POISON).all() and (r.idx[r.nv:] == POISON).all()
    assert (r.tri[r.nt:] == POISON).all()


def sphere(n, seed=5, dtype=np.float64):
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(dtype)


@functools.lru_cache(maxsize=None)
def sphere_oracle(n):
    return orc.convex_hull(sphere(n))


# ---- goldens ------------------------------------------------------------------------
def _golden_hpr(g):
    return (tuple(g["camera"]), float(g["radius"])) if "camera" in g else None


@pytest.mark.parametrize("index", [np.int32, np.int64])
@pytest.mark.parametrize("name", GOLDENS)
def test_golden_abi(name, index):
    g = golden(name)
    r = call_abi(g["points"], index, _golden_hpr(g))
    expect(r, g["points"], g["point_indices"], g["triangles"], index)


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_python(name):
    from open3d_amd import pointcloud, trianglemesh
    g = golden(name)
    p = _dev(g["points"])
    if "camera" in g:
        mesh, idx = pointcloud.hidden_point_removal(
            {"positions": p}, g["camera"].tolist(), float(g["radius"]))
        assert idx.dtype == torch.int64
        assert mesh["indices"].dtype == torch.int64
        meshes = [(mesh, idx)]
    else:
        a = pointcloud.compute_convex_hull({"positions": p})
        b = trianglemesh.compute_convex_hull({"positions": p})
        meshes = [(a, a["point_indices"]), (b, b["point_indices"])]
        for m, idx in meshes:
            assert idx.dtype == torch.int32
            assert m["indices"].dtype == torch.int32
    for m, idx in meshes:
        assert np.array_equal(idx.cpu().numpy(), g["point_indices"])
        assert np.array_equal(m["indices"].cpu().numpy(), g["triangles"])
        assert np.array_equal(_bits(m["positions"].cpu().numpy()),
                              _bits(g["points"][g["point_indices"]]))


# ---- smallest shapes ----------------------------------------------------------------
EDGE_SIZES = [4, 5, 8, 64, 65, HULL_BLOCK - 1, HULL_BLOCK, HULL_BLOCK + 1,
              SCAN_TILE - 1, SCAN_TILE + 1]


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_sphere_sizes_against_the_oracle(n):
    pts = sphere(n)
    idx, tri = sphere_oracle(n)
    assert len(idx) == n
    expect(call_abi(pts), pts, idx, tri)


def test_float32_sphere_against_the_oracle():
    pts = sphere(HULL_BLOCK + 1, seed=6, dtype=np.float32)
    idx, tri = orc.convex_hull(pts)
    expect(call_abi(pts, np.int64), pts, idx, tri, np.int64)


# ---- conflict-heavy rounds ----------------------------------------------------------
def test_sphere_20000_every_point_is_a_vertex():
    n = 20000
    pts = sphere(n, seed=8)
    r = call_abi(pts)
    assert r.status == OK and r.nv == n and r.nt == 2 * n - 4
    assert np.array_equal(r.idx, np.arange(n))
    tri = r.tri.astype(np.int64)
    assert (tri[:, 0] < tri[:, 1]).all() and (tri[:, 0] < tri[:, 2]).all()
    order = np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))
    assert np.array_equal(order, np.arange(len(tri)))
    assert orc.edges_closed_and_oriented(tri) and orc.euler(tri) == 2
    # no point above any facet: 1e-9 E is the goldens' margin, four orders
    # above eps and the rounding of this check
    P = _dev(pts)
    T = _dev(tri)
    a, b, c = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    nrm = torch.linalg.cross(b - a, c - a)
    nrm = nrm / nrm.norm(dim=1, keepdim=True)
    off = (a * nrm).sum(dim=1)
    worst = max(float((P[k:k + 2000] @ nrm.T - off[None, :]).max())
                for k in range(0, n, 2000))
    assert worst <= 1e-9 * 2.0


# ---- exact degenerate inputs --------------------------------------------------------
LATTICE = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"),
                   -1).reshape(-1, 3)


def _faces_cloud(order):
    on_face = LATTICE[((LATTICE == 0) | (LATTICE == 5)).any(axis=1)]
    corner = ((on_face == 0) | (on_face == 5)).all(axis=1)
    rng = np.random.default_rng(21)
    inner = on_face[~corner]
    pick = inner[rng.integers(0, len(inner), 500)]  # with repeats
    cloud = np.concatenate([on_face[corner], pick])
    if order == 1:
        cloud = cloud[::-1]
    elif order == 2:
        cloud = cloud[rng.permutation(len(cloud))]
    return np.ascontiguousarray(cloud)


def check_exact_cube(pts, r):
    """The validity properties of the hull of integer points that fill the
    cube [0, 5]^3, in integers."""
    assert r.status == OK
    idx, tri = r.idx[:r.nv].astype(np.int64), r.tri[:r.nt].astype(np.int64)
    P = pts.astype(np.int64)
    T = idx[tri]
    a, b, c = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    n = np.cross(b - a, c - a)
    above = np.einsum("fk,pfk->pf", n, P[:, None, :] - a[None, :, :])
    assert (above <= 0).all()
    assert orc.edges_closed_and_oriented(tri) and orc.euler(tri) == 2
    assert six_volume(P, idx, tri) == 6 * 5 ** 3
    corners = {tuple(x) for x in P[idx] if all(v in (0, 5) for v in x)}
    assert len(corners) == 8
    assert np.array_equal(_bits(r.pos[:r.nv]), _bits(pts[idx]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lattice(dtype):
    pts = LATTICE.astype(dtype)
    check_exact_cube(pts, call_abi(pts))


@pytest.mark.parametrize("order", [0, 1, 2])
def test_cube_corners_and_face_points(order):
    pts = _faces_cloud(order)
    check_exact_cube(pts, call_abi(pts))


def test_cloud_repeated_twice():
    pts = LATTICE[np.random.default_rng(3).permutation(len(LATTICE))]
    one = call_abi(pts)
    two = call_abi(np.concatenate([pts, pts]))
    check_exact_cube(np.concatenate([pts, pts]), two)
    assert (two.idx[:two.nv] < len(pts)).all()
    assert (one.nv, one.nt) == (two.nv, two.nt)
    assert np.array_equal(one.idx[:one.nv], two.idx[:two.nv])
    assert np.array_equal(one.tri[:one.nt], two.tri[:two.nt])
    s = sphere(300, seed=4)
    idx, tri = orc.convex_hull(s)
    expect(call_abi(np.concatenate([s, s])), np.concatenate([s, s]), idx, tri)


# ---- hidden-point removal -----------------------------------------------------------
def test_hpr_sphere_seen_from_outside():
    n = 2000
    pts = sphere(n, seed=12)
    # 100 x the sphere's diameter. (The operator itself, Qhull included,
    # starts to keep far-side points once the radius is so large that the
    # flipped shell is thinner than its facets' sagitta: 74 of them at
    # radius 5000 for this cloud, none at 50 to 500.)
    camera, radius = (0.0, 0.0, 5.0), 200.0
    r = call_abi(pts, np.int64, (camera, radius))
    idx, tri = orc.hidden_point_removal(pts, camera, radius)
    expect(r, pts, idx, tri, np.int64)
    # only points of the half that faces the camera
    assert 0 < r.nv < n and (pts[r.idx[:r.nv], 2] > 0).all()
    # the origin (point n) and its triangles are gone
    assert (r.idx[:r.nv] < n).all() and (r.tri[:r.nt] < r.nv).all()
    assert r.nt < 2 * r.nv - 4


def test_hpr_camera_inside_a_sphere_keeps_every_point():
    n = 1000
    pts = sphere(n, seed=13, dtype=np.float32)
    r = call_abi(pts, np.int32, ((0.1, -0.05, 0.02), 1000.0))
    assert r.status == OK and r.nv == n and r.nt == 2 * n - 4
    assert np.array_equal(r.idx, np.arange(n))
    assert np.array_equal(_bits(r.pos), _bits(pts))
    idx, tri = orc.hidden_point_removal(pts, (0.1, -0.05, 0.02), 1000.0)
    expect(r, pts, idx, tri)


def test_hpr_three_points():
    pts = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    r = call_abi(pts, np.int64, ((0.0, 0.0, 0.0), 10.0), tcap=4)
    idx, tri = orc.hidden_point_removal(pts, (0.0, 0.0, 0.0), 10.0)
    assert len(idx) == 3 and len(tri) == 1
    expect(r, pts, idx, tri, np.int64)


# ---- protocol -----------------------------------------------------------------------
def test_count_only_and_capacity():
    pts = sphere(100, seed=14)
    idx, tri = orc.convex_hull(pts)
    r = call_abi(pts, vcap=-1, tcap=0)
    assert (r.status, r.nv, r.nt) == (OK, len(idx), len(tri))
    for vcap, tcap in ((len(idx) - 1, len(tri)), (len(idx), len(tri) - 1)):
        r = call_abi(pts, vcap=vcap, tcap=tcap)
        assert (r.status, r.nv, r.nt) == (CAPACITY, len(idx), len(tri))
        assert (r.pos == POISON).all() and (r.idx == POISON).all()
        assert (r.tri == POISON).all()
    expect(call_abi(pts, vcap=len(idx), tcap=len(tri)), pts, idx, tri)


@pytest.mark.parametrize("name", sorted(refusal_cases()))
def test_refusals_leave_the_outputs_untouched(name):
    points, camera, radius, status = refusal_cases()[name]
    hpr = None if camera is None else (camera, radius)
    for dtype in (np.float64, np.float32):
        if name == "point_at_camera" and dtype == np.float32:
            hpr = (tuple(float(v) for v in points.astype(dtype)[7]), radius)
        r = call_abi(points.astype(dtype), np.int32, hpr, vcap=len(points),
                     tcap=2 * len(points))
        assert r.status == status, name
        assert (r.nv, r.nt) == (-5, -5)
        assert (r.pos == POISON).all() and (r.idx == POISON).all()
        assert (r.tri == POISON).all()


def test_argument_refusals():
    L = _L()
    pts = sphere(10)
    p = _dev(pts)
    nv, nt = C.c_int64(0), C.c_int64(0)
    call = L.lib().o3dmi_pointcloud_convex_hull
    tail = (None, None, -1, None, 0, 4, C.byref(nv), C.byref(nt), None)
    assert call(L.ptr(p), 10, 1, *tail) == OK
    assert call(None, 10, 1, *tail) == INVALID_ARG
    assert call(L.ptr(p), 3, 1, *tail) == INVALID_ARG
    assert call(L.ptr(p), 2 ** 31 - 1, 1, *tail) == INVALID_ARG
    assert call(L.ptr(p), 10, 4, *tail) == INVALID_ARG
    assert call(L.ptr(p), 10, 1, None, None, -1, None, 0, 0, C.byref(nv),
                C.byref(nt), None) == INVALID_ARG
    assert call(L.ptr(p), 10, 1, None, None, -1, None, 0, 4, None,
                C.byref(nt), None) == INVALID_ARG
    hpr = L.lib().o3dmi_pointcloud_hidden_point_removal
    cam = (C.c_double * 3)(0.0, 0.0, 3.0)
    assert hpr(L.ptr(p), 10, 1, cam, C.c_double(10.0), *tail) == OK
    assert hpr(L.ptr(p), 10, 1, None, C.c_double(10.0), *tail) == INVALID_ARG
    assert hpr(L.ptr(p), 2, 1, cam, C.c_double(10.0), *tail) == INVALID_ARG
    assert hpr(L.ptr(p), 10, 1, cam, C.c_double(-1.0), *tail) == INVALID_ARG
    bad = (C.c_double * 3)(0.0, float("nan"), 3.0)
    assert hpr(L.ptr(p), 10, 1, bad, C.c_double(10.0), *tail) == INVALID_ARG


def test_python_layer_errors():
    from open3d_amd import pointcloud
    flat = _dev(np.concatenate([sphere(50)[:, :2], np.zeros((50, 1))], 1))
    with pytest.raises(_L().O3DMIError) as e:
        pointcloud.compute_convex_hull({"positions": flat})
    assert e.value.status == SINGULAR
    with pytest.raises(ValueError, match="joggle"):
        pointcloud.compute_convex_hull({"positions": flat}, True)


# ---- determinism --------------------------------------------------------------------
def _stats():
    out = (C.c_int64 * 4)()
    assert _L().lib().o3dmi_internal_pointcloud_hull_stats(out) == OK
    return list(out)


def test_same_bits_three_times_and_in_every_form(monkeypatch):
    pts = sphere(3000, seed=15)
    cube = np.random.default_rng(16).random((5000, 3)).astype(np.float32)
    for cloud in (pts, cube):
        first = call_abi(cloud)
        rounds, sweeps, winners, _ = _stats()
        assert first.status == OK and sweeps == 0 and winners > rounds
        for _ in range(2):
            again = call_abi(cloud)
            assert (again.nv, again.nt) == (first.nv, first.nt)
            assert np.array_equal(again.idx, first.idx)
            assert np.array_equal(again.tri, first.tri)
            assert np.array_equal(_bits(again.pos), _bits(first.pos))
        # a walk of at most 3 facets: the best candidate often sees more, and
        # those rounds fall back to the sweep form
        monkeypatch.setenv("O3DMI_HULL_WALK", "3")
        short = call_abi(cloud)
        assert 0 < _stats()[1] < _stats()[0]
        monkeypatch.delenv("O3DMI_HULL_WALK")
        forms = [short]
        if cloud is cube:  # few vertices: one insertion per round is quick
            monkeypatch.setenv("O3DMI_HULL_WALK", "sweep")
            forms.append(call_abi(cloud))
            assert _stats()[0] == _stats()[1] == _stats()[2]
            monkeypatch.delenv("O3DMI_HULL_WALK")
        for other in forms:
            assert (other.status, other.nv, other.nt) == (OK, first.nv,
                                                          first.nt)
            assert np.array_equal(other.idx, first.idx)
            assert np.array_equal(other.tri, first.tri)
    assert 3 < WALK_CAP


def test_non_default_stream():
    pts = sphere(500, seed=17)
    idx, tri = orc.convex_hull(pts)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r = call_abi(pts)
    expect(r, pts, idx, tri)
