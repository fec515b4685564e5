"""GPU tests of TriangleMesh sampling, the closest-point queries and
TriangleMesh::ComputeMetrics against the numpy restatement
(tests/_mesh_distance_oracle.py: it never builds a tree) and upstream's
literal vectors (tests/golden/mesh_distance_vectors.json). Every comparison
is bit for bit unless a tolerance is named; outputs are poisoned first."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mesh_distance_oracle as orc

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED = 0, 1, 7
F32C, F64C, U16C, U8C, I32C, I64C = 0, 1, 2, 3, 4, 5
CODE = {np.float32: F32C, np.float64: F64C, np.int32: I32C, np.int64: I64C,
        np.uint8: U8C, np.uint16: U16C}
F32 = np.float32
POISON = -777.0
POISON_ID = 0x5A5A5A5A
CHAMFER, HAUSDORFF, FSCORE = 0, 1, 2


def _L():
    from open3d_amd import _lib
    return _lib


def _tm():
    from open3d_amd import trianglemesh
    return trianglemesh


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32,
                   8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.size == 0:
        return
    differ = (_bits(got) != _bits(want)).reshape(got.shape[0], -1).any(axis=1)
    bad = np.flatnonzero(differ)
    assert len(bad) == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _poison(shape, dtype=torch.float32):
    return torch.full(shape, POISON, dtype=dtype, device="cuda")


TCODE = {torch.float32: F32C, torch.float64: F64C, torch.int32: I32C,
         torch.int64: I64C}


def _mesh_args(p, t):
    L = _L()
    return (L.ptr(p), p.shape[0], TCODE[p.dtype], L.ptr(t), t.shape[0],
            TCODE[t.dtype])


@pytest.fixture(scope="module")
def gold():
    return orc.golden()


# ---- sampling --------------------------------------------------------------------
def abi_sample(pos, tri, n, seed, vn=None, tn=None, colors=None,
               want_normals=None, want_colors=None):
    L = _L()
    pd, td = _dev(pos), _dev(tri)
    fdt = pd.dtype
    vnd = _dev(vn) if vn is not None else None
    tnd = _dev(tn) if tn is not None else None
    cd = _dev(colors) if colors is not None else None
    if want_normals is None:
        want_normals = vn is not None or tn is not None
    if want_colors is None:
        want_colors = colors is not None
    rows = max(n, 1)
    points = _poison((rows, 3), fdt)
    normals = _poison((rows, 3), fdt) if want_normals else None
    cols = _poison((rows, 3)) if want_colors else None
    tris = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    st = L.lib().o3dmi_trianglemesh_sample_points_uniformly(
        L.ptr(pd), len(pos), CODE[pos.dtype.type], L.ptr(td), len(tri),
        CODE[tri.dtype.type], n, seed, L.ptr(vnd), L.ptr(tnd), L.ptr(cd),
        CODE[colors.dtype.type] if colors is not None else 0, L.ptr(points),
        L.ptr(normals), L.ptr(cols), L.ptr(tris), None)
    out = dict(points=points.cpu().numpy(), triangles=tris.cpu().numpy())
    if normals is not None:
        out["normals"] = normals.cpu().numpy()
    if cols is not None:
        out["colors"] = cols.cpu().numpy()
    return st, out


def _untouched(out):
    assert (out["points"] == POISON).all()
    assert (out["triangles"] == -7).all()
    for k in ("normals", "colors"):
        assert k not in out or (out[k] == POISON).all()


def sample_mesh(m, fdt, idt, seed):
    """A soup of m triangles over ~m / 2 + 3 vertices with areas from 0 up:
    every fourth triangle is degenerate, and with more than two groups the
    whole second group of 512 is."""
    rng = np.random.default_rng(seed)
    v = m // 2 + 3
    pos = rng.standard_normal((v, 3)).astype(fdt)
    tri = rng.integers(0, v, (m, 3)).astype(idt)
    if m < 4:  # too few to leave the total area to chance
        tri = (np.arange(m)[:, None] + np.arange(3)[None, :]).astype(idt)
    else:
        tri[1::4, 2] = tri[1::4, 1]  # zero area, interleaved
    if m > 1024:
        tri[512:1024, 1] = tri[512:1024, 0]  # a whole group of zeros
    return pos, tri


SAMPLE_SIZES = [1, 2, 512, 513, 262145]  # 262145: three levels of the tree
SAMPLE_DTYPES = [(np.float32, np.int32), (np.float64, np.int64),
                 (np.float32, np.int64), (np.float64, np.int32)]


@pytest.mark.parametrize("fdt,idt", SAMPLE_DTYPES)
@pytest.mark.parametrize("m", SAMPLE_SIZES)
def test_sampling_is_the_restatement(m, fdt, idt):
    pos, tri = sample_mesh(m, fdt, idt, seed=m)
    want = orc.sample(pos, tri, 1000, 9)
    if m > 1024:
        assert len(orc.prefix_levels(orc.tm.triangle_areas(pos, tri))) == 3
    for n in (1, 2, 1000):
        st, got = abi_sample(pos, tri, n, 9)
        assert st == OK
        _same(got["triangles"], want["triangles"][:n], "triangles")
        _same(got["points"], want["points"][:n], "points")
    areas = orc.tm.triangle_areas(pos, tri)
    assert (areas[want["triangles"]] > 0).all()


@pytest.mark.parametrize("fdt", [np.float32, np.float64])
@pytest.mark.parametrize("color_dt", [np.float32, np.uint8, np.uint16])
def test_sampling_mixes_normals_and_colours(fdt, color_dt):
    pos, tri = sample_mesh(513, fdt, np.int32, seed=21)
    rng = np.random.default_rng(22)
    vn = rng.standard_normal(pos.shape).astype(fdt)
    tn = rng.standard_normal((len(tri), 3)).astype(fdt)
    if color_dt == np.float32:
        colors = rng.random(pos.shape).astype(np.float32)
    else:
        colors = rng.integers(0, np.iinfo(color_dt).max + 1,
                              pos.shape).astype(color_dt)
    n = 1000
    want = orc.sample(pos, tri, n, 4, vertex_normals=vn, vertex_colors=colors)
    st, got = abi_sample(pos, tri, n, 4, vn=vn, tn=tn, colors=colors)
    assert st == OK
    for k in ("triangles", "points", "normals", "colors"):
        _same(got[k], want[k], k)
    # triangle normals are copied when no vertex normals are given
    want = orc.sample(pos, tri, n, 4, triangle_normals=tn)
    st, got = abi_sample(pos, tri, n, 4, tn=tn)
    assert st == OK
    _same(got["normals"], want["normals"], "triangle normals")
    _same(got["points"], want["points"], "points")


def test_sampling_python_mirror():
    tm = _tm()
    pos, tri = sample_mesh(65, np.float32, np.int64, seed=31)
    rng = np.random.default_rng(32)
    vn = rng.standard_normal(pos.shape).astype(F32)
    colors = rng.integers(0, 256, pos.shape).astype(np.uint8)
    mesh = {"positions": _dev(pos), "indices": _dev(tri)}
    out = tm.sample_points_uniformly(mesh, 100, seed=3)
    assert set(out) == {"positions"}
    _same(out["positions"].cpu().numpy(),
          orc.sample(pos, tri, 100, 3)["points"])
    mesh.update(normals=_dev(vn), colors=_dev(colors))
    out = tm.sample_points_uniformly(mesh, 100, seed=3)
    want = orc.sample(pos, tri, 100, 3, vertex_normals=vn,
                      vertex_colors=colors)
    _same(out["normals"].cpu().numpy(), want["normals"])
    _same(out["colors"].cpu().numpy(), want["colors"])
    # use_triangle_normal: computed first (normalised), then copied
    out = tm.sample_points_uniformly(mesh, 100, use_triangle_normal=True,
                                     seed=3)
    tn = orc.tm.normalize_normals(orc.tm.triangle_normals(pos, tri))
    want = orc.sample(pos, tri, 100, 3, triangle_normals=tn)
    _same(out["normals"].cpu().numpy(), want["normals"])
    with pytest.raises(ValueError):
        tm.sample_points_uniformly(mesh, 0)


def test_sampling_seeds():
    pos, tri = sample_mesh(513, np.float32, np.int32, seed=41)
    _, a = abi_sample(pos, tri, 1000, 5)
    _, b = abi_sample(pos, tri, 1000, 5)
    _, c = abi_sample(pos, tri, 1000, 6)
    _same(a["points"], b["points"])
    _same(a["triangles"], b["triangles"])
    assert not np.array_equal(a["points"], c["points"])


def test_sampling_follows_the_areas(gold):
    g = gold["area_ratio"]
    pos, tri = np.array(g["positions"], F32), np.array(g["triangles"],
                                                       np.int32)
    n = g["n"]
    st, got = abi_sample(pos, tri, n, g["seed"])
    assert st == OK
    first = int(np.count_nonzero(got["triangles"] == 0))
    sigma = np.sqrt(n * 0.25 * 0.75)  # ~137: within 685 of 25000
    assert abs(first - n / 4) <= 5 * sigma, first
    # every point lies on its triangle's plane z = 0 or z = 5 (the three
    # weights add up to 1 within a few float32 roundings)
    z = got["points"][:, 2]
    want_z = np.where(got["triangles"] == 0, F32(0), F32(5))
    assert np.abs(z - want_z).max() <= 5 * 8 * np.finfo(F32).eps


def test_sampling_errors_leave_the_outputs_alone():
    pos, tri = sample_mesh(65, np.float32, np.int32, seed=51)
    st, out = abi_sample(pos, tri, 0, 1)
    assert st == INVALID_ARG
    _untouched(out)
    st, out = abi_sample(pos, tri, -3, 1)
    assert st == INVALID_ARG
    _untouched(out)
    flat = tri.copy()
    flat[:, 2] = flat[:, 1]  # total area 0
    st, out = abi_sample(pos, flat, 10, 1)
    assert st == INVALID_ARG
    _untouched(out)
    bad = pos.copy()
    bad[tri[7, 0], 1] = np.nan  # a NaN vertex of a referenced triangle
    st, out = abi_sample(bad, tri, 10, 1)
    assert st == INVALID_ARG
    _untouched(out)
    far = tri.copy()
    far[3, 1] = len(pos)  # an index out of range
    st, out = abi_sample(pos, far, 10, 1)
    assert st == INVALID_ARG
    _untouched(out)
    far[3, 1] = -1
    st, out = abi_sample(pos, far, 10, 1)
    assert st == INVALID_ARG
    _untouched(out)
    # normals wanted, none given
    st, out = abi_sample(pos, tri, 10, 1, want_normals=True)
    assert st == INVALID_ARG
    _untouched(out)


# ---- closest points --------------------------------------------------------------
KEYS = ("points", "primitive_ids", "primitive_uvs", "primitive_normals",
        "distance")


class Outputs:
    def __init__(self, q):
        rows = max(q, 1)
        self.t = dict(
            points=_poison((rows, 3)),
            primitive_ids=torch.full((rows,), POISON_ID, dtype=torch.int32,
                                     device="cuda"),
            primitive_uvs=_poison((rows, 2)),
            primitive_normals=_poison((rows, 3)),
            distance=_poison((rows,)))
        self.q = q

    def ptrs(self):
        return tuple(_L().ptr(self.t[k]) for k in KEYS)

    def numpy(self):
        out = {k: v.cpu().numpy() for k, v in self.t.items()}
        out["primitive_ids"] = out["primitive_ids"].view(np.uint32)
        return out

    def untouched(self):
        out = self.numpy()
        assert (out["primitive_ids"] == POISON_ID).all()
        for k in KEYS:
            if k != "primitive_ids":
                assert (out[k] == POISON).all(), k


class Handle:
    def __init__(self, pos, tri):
        self.pd, self.td = _dev(pos), _dev(tri)
        self.h = C.c_void_p()
        self.status = _L().lib().o3dmi_mesh_bvh_create(
            *_mesh_args(self.pd, self.td), C.byref(self.h), None)

    def query(self, queries, order=None):
        """order None: the public call; 0 / 1: the internal call with the
        queries taken in input / Morton order."""
        L = _L()
        qd = _dev(queries)
        out = Outputs(len(queries))
        if order is None:
            st = L.lib().o3dmi_mesh_bvh_closest_points(
                self.h, L.ptr(qd), len(queries), CODE[queries.dtype.type],
                *out.ptrs(), None)
        else:
            st = L.lib().o3dmi_internal_mesh_bvh_query(
                self.h, L.ptr(qd), len(queries), *out.ptrs(), order, None,
                None)
        return st, out

    def close(self):
        assert _L().lib().o3dmi_mesh_bvh_destroy(self.h) == OK
        self.h = C.c_void_p()


def one_shot(pos, tri, queries):
    L = _L()
    pd, td, qd = _dev(pos), _dev(tri), _dev(queries)
    out = Outputs(len(queries))
    st = L.lib().o3dmi_trianglemesh_closest_points(
        *_mesh_args(pd, td), L.ptr(qd), len(queries), *out.ptrs(), None)
    return st, out


def check_queries(pos, tri, queries, orders=(None, 0, 1)):
    want = orc.closest_points(pos, tri, queries)
    h = Handle(pos, tri)
    assert h.status == OK
    for order in orders:
        st, out = h.query(queries, order)
        assert st == OK
        got = out.numpy()
        for k in KEYS:
            _same(got[k], want[k], "%s (order %r)" % (k, order))
    h.close()
    return want


def soup(m, seed, offset=0.0, spoil=False):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (m, 1, 3))
    pos = (centres + 0.2 * rng.standard_normal((m, 3, 3))).reshape(-1, 3)
    pos = (pos + offset).astype(F32)
    tri = np.arange(3 * m, dtype=np.int32).reshape(m, 3)
    if spoil:  # degenerate and sliver triangles mixed in
        for t in range(0, m, 5):
            pos[3 * t + 1] = pos[3 * t]  # a == b
        for t in range(1, m, 5):  # collinear
            pos[3 * t + 2] = pos[3 * t] + F32(2) * (pos[3 * t + 1] -
                                                    pos[3 * t])
        for t in range(2, m, 5):  # sliver
            mid = F32(0.5) * (pos[3 * t] + pos[3 * t + 1])
            pos[3 * t + 2] = mid + F32(1e-4) * rng.standard_normal(3).astype(
                F32)
        for t in range(3, m, 25):  # a point
            pos[3 * t + 1] = pos[3 * t + 2] = pos[3 * t]
    return pos, tri


def mixed_queries(pos, tri, q, seed, offset=0.0):
    """Mesh vertices, points on the surface, points 1e6 away, random points."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(q):
        kind = i % 4
        if kind == 0:
            rows.append(pos[tri[rng.integers(len(tri)), rng.integers(3)]])
        elif kind == 1:
            a, b, c = (pos[k] for k in tri[rng.integers(len(tri))])
            w = rng.dirichlet(np.ones(3)).astype(F32)
            rows.append(w[0] * a + w[1] * b + w[2] * c)
        elif kind == 2 and i % 8 == 2:
            rows.append(1e6 * rng.standard_normal(3))
        else:
            rows.append(offset + rng.uniform(-1.5, 1.5, 3))
    return np.array(rows, F32).reshape(q, 3)


@pytest.mark.parametrize("q", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("m", [1, 2, 3, 64, 65, 8193])
def test_closest_points_on_a_soup(m, q):
    if m == 8193:
        q = min(q, 257)  # keeps the exhaustive restatement quick
    pos, tri = soup(m, seed=m)
    check_queries(pos, tri, mixed_queries(pos, tri, q, seed=q))


def test_closest_points_on_the_cube(gold):
    pos, tri = orc.unit_cube()
    g = gold["cube"]
    mid = [[x, y, z] for x in (0, 0.5, 1) for y in (0, 0.5, 1)
           for z in (0, 0.5, 1)]  # vertices, edge and face midpoints, centre
    queries = np.array(g["queries"] + mid, F32)
    queries = np.concatenate([queries, mixed_queries(pos, tri, 200, seed=2)])
    want = check_queries(pos, tri, queries)
    np.testing.assert_allclose(want["distance"][:3], np.array(g["distance"]),
                               rtol=g["rtol"])
    centre = 3 + mid.index([0.5, 0.5, 0.5])
    assert want["primitive_ids"][centre] == 0  # all twelve at 0.5
    assert want["distance"][centre] == 0.5


def test_upstream_closest_point_vectors(gold):
    g = gold["closest_points"]
    pos = np.array(g["positions"], F32)
    tri = np.array(g["triangles"], np.int64)
    st, out = one_shot(pos, tri, np.array(g["queries"], F32))
    assert st == OK
    got = out.numpy()
    np.testing.assert_allclose(got["points"], np.array(g["points"]),
                               rtol=g["rtol"], atol=g["atol"])
    assert list(got["primitive_ids"]) == g["primitive_ids"]


def planar_grid(n):
    xs = np.arange(n + 1, dtype=F32) / F32(n)
    pos = np.array([[x, y, 0] for y in xs for x in xs], F32)
    tri = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            tri += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    return pos, np.array(tri, np.int32)


def test_closest_points_on_a_planar_grid():
    pos, tri = planar_grid(9)  # zero extent on z
    queries = mixed_queries(pos, tri, 300, seed=3)
    check_queries(pos, tri, queries)


def test_identical_triangles_tie_to_index_zero():
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
    tri = np.tile(np.array([[0, 1, 2]], np.int32), (100, 1))
    queries = mixed_queries(pos, tri, 130, seed=4)
    want = check_queries(pos, tri, queries)
    assert (want["primitive_ids"] == 0).all()


def test_every_vertex_at_one_point():
    pos = np.tile(np.array([[0.25, -1.5, 3.0]], F32), (30, 1))
    tri = np.arange(30, dtype=np.int32).reshape(10, 3)
    queries = mixed_queries(pos, tri, 70, seed=5)
    want = check_queries(pos, tri, queries)
    assert (want["primitive_ids"] == 0).all()
    assert np.isfinite(want["distance"]).all()


@pytest.mark.parametrize("m", [65, 500])
def test_degenerate_and_sliver_triangles(m):
    pos, tri = soup(m, seed=6, spoil=True)
    queries = mixed_queries(pos, tri, 400, seed=7)
    check_queries(pos, tri, queries)


def test_a_mesh_of_nan_pairs_gives_the_empty_row():
    # a == b and the query between a and c: every pair is NaN
    pos = np.array([[0, 0, 0], [0, 0, 0], [2, 0, 0]], F32)
    tri = np.array([[0, 1, 2], [0, 1, 2]], np.int32)
    queries = np.array([[1, 1, 0], [-1, 1, 0], [0.5, 0, 0.25]], F32)
    want = check_queries(pos, tri, queries)
    assert list(want["primitive_ids"]) == [orc.NO_TRIANGLE, 0,
                                           orc.NO_TRIANGLE]
    assert want["distance"][0] == np.inf and not want["points"][0].any()


def test_soup_offset_by_1e4():
    pos, tri = soup(300, seed=8, offset=1e4)
    queries = mixed_queries(pos, tri, 300, seed=9, offset=1e4)
    check_queries(pos, tri, queries)


def test_refit_at_a_size_that_spans_the_chip():
    """The refit hands boxes from thread to thread inside one launch; with a
    quarter of a million leaves the climbers run on every compute unit at
    once. A box read too early would be too small and prune a winner."""
    pos, tri = soup(262145, seed=18)
    queries = mixed_queries(pos, tri, 16, seed=19)
    check_queries(pos, tri, queries, orders=(0,))


def test_handle_one_shot_distance_and_python_mirror():
    tm = _tm()
    L = _L()
    pos, tri = soup(65, seed=10)
    queries = mixed_queries(pos, tri, 120, seed=11)
    want = orc.closest_points(pos, tri, queries)
    h = Handle(pos, tri)
    assert h.status == OK
    # the handle owns its copies: the mesh may go
    h.pd.fill_(0)
    h.td.fill_(0)
    _, first = h.query(queries)
    _, second = h.query(queries)
    for k in KEYS:
        _same(first.numpy()[k], want[k], k)
        _same(second.numpy()[k], first.numpy()[k], k)
    # q == 0 writes nothing
    st, out = h.query(queries[:0])
    assert st == OK
    out.untouched()
    h.close()
    st, out = one_shot(pos, tri, queries)
    assert st == OK
    for k in KEYS:
        _same(out.numpy()[k], want[k], k)
    pd, td, qd = _dev(pos), _dev(tri), _dev(queries)
    dist = _poison((len(queries),))
    assert L.lib().o3dmi_trianglemesh_compute_distance(
        *_mesh_args(pd, td), L.ptr(qd), len(queries), L.ptr(dist),
        None) == OK
    _same(dist.cpu().numpy(), want["distance"])
    # the mirror keeps the leading query dimensions
    bvh = tm.MeshBVH({"positions": pd, "indices": td})
    shaped = qd.reshape(4, 30, 3)
    got = bvh.compute_closest_points(shaped)
    assert set(got) == {"points", "geometry_ids", "primitive_ids",
                        "primitive_uvs", "primitive_normals"}
    assert got["points"].shape == (4, 30, 3)
    assert got["primitive_ids"].shape == (4, 30)
    assert got["primitive_uvs"].shape == (4, 30, 2)
    assert got["primitive_normals"].shape == (4, 30, 3)
    _same(got["points"].reshape(-1, 3).cpu().numpy(), want["points"])
    ids = got["primitive_ids"].reshape(-1).cpu().numpy().view(np.uint32)
    _same(ids, want["primitive_ids"])
    d = bvh.compute_distance(shaped)
    assert d.shape == (4, 30)
    _same(d.reshape(-1).cpu().numpy(), want["distance"])
    bvh.close()


def test_closest_point_errors_leave_the_outputs_alone():
    L = _L()
    pos, tri = soup(20, seed=12)
    queries = mixed_queries(pos, tri, 10, seed=13)
    bad_q = queries.copy()
    bad_q[4, 1] = np.nan
    h = Handle(pos, tri)
    st, out = h.query(bad_q)
    assert st == INVALID_ARG
    out.untouched()
    st, out = h.query(queries.astype(np.float64))
    assert st == UNSUPPORTED
    out.untouched()
    h.close()
    bad_p = pos.copy()
    bad_p[7, 2] = np.inf
    assert Handle(bad_p, tri).status == INVALID_ARG
    st, out = one_shot(bad_p, tri, queries)
    assert st == INVALID_ARG
    out.untouched()
    far = tri.copy()
    far[5, 0] = len(pos)
    assert Handle(pos, far).status == INVALID_ARG
    st, out = one_shot(pos, far, queries)
    assert st == INVALID_ARG
    out.untouched()
    st, out = one_shot(pos, tri[:0], queries)  # m == 0
    assert st == INVALID_ARG
    out.untouched()
    pd, td, qd = _dev(pos.astype(np.float64)), _dev(tri), _dev(queries)
    out = Outputs(len(queries))
    st = L.lib().o3dmi_trianglemesh_closest_points(
        *_mesh_args(pd, td), L.ptr(qd), len(queries), *out.ptrs(), None)
    assert st == UNSUPPORTED
    out.untouched()


# ---- metrics ---------------------------------------------------------------------
def abi_metrics(mesh1, mesh2, metrics, radii, n, seed=0, capacity=None):
    L = _L()
    (p1, t1), (p2, t2) = mesh1, mesh2
    d = [_dev(x) for x in (p1, t1, p2, t2)]
    n_values = sum(len(radii) if m == FSCORE else 1 for m in metrics)
    cap = n_values if capacity is None else capacity
    values = (C.c_float * max(cap, 1))(*([POISON] * max(cap, 1)))
    counts = (C.c_int64 * max(2 * len(radii), 1))(
        *([-7] * max(2 * len(radii), 1)))
    raw = L.MetricsRawC()
    raw.counts = C.cast(counts, C.POINTER(C.c_int64))
    st = L.lib().o3dmi_trianglemesh_compute_metrics(
        L.ptr(d[0]), len(p1), L.ptr(d[1]), len(t1), CODE[t1.dtype.type],
        L.ptr(d[2]), len(p2), L.ptr(d[3]), len(t2), CODE[t2.dtype.type],
        CODE[p1.dtype.type], (C.c_int * max(len(metrics), 1))(*metrics),
        len(metrics), (C.c_float * max(len(radii), 1))(*radii), len(radii),
        n, seed, values, cap, C.byref(raw), None)
    r = len(radii)
    return st, np.array(list(values)[:n_values], F32), dict(
        sum=list(raw.sum), max=list(raw.max),
        counts=[list(counts)[:r], list(counts)[r:2 * r]],
        second_pass_queries=list(raw.second_pass_queries))


def test_metrics_are_the_restated_chain():
    mesh1, mesh2 = soup(300, seed=14), soup(300, seed=15)
    mesh2 = (mesh2[0], mesh2[1].astype(np.int64))
    metrics, radii = [CHAMFER, HAUSDORFF, FSCORE], [0.02, 0.1, 0.5]
    want, want_raw = orc.compute_metrics(mesh1, mesh2, metrics, radii, 1000,
                                         seed=3)
    st, got, raw = abi_metrics(mesh1, mesh2, metrics, radii, 1000, seed=3)
    assert st == OK
    _same(got, want, "values")
    assert [np.float64(x).tobytes() for x in raw["sum"]] == \
        [np.float64(x).tobytes() for x in want_raw["sum"]]
    assert raw["max"] == [float(x) for x in want_raw["max"]]
    assert raw["counts"] == want_raw["counts"]
    assert raw["second_pass_queries"] == [0, 0]
    # FScore listed twice expands twice, as the cloud call does
    st, twice, _ = abi_metrics(mesh1, mesh2, [FSCORE, CHAMFER, FSCORE], radii,
                               1000, seed=3)
    assert st == OK
    _same(twice, np.concatenate([want[2:], want[:1], want[2:]]))
    # the mirror
    tm = _tm()
    m1 = {"positions": _dev(mesh1[0]), "indices": _dev(mesh1[1])}
    m2 = {"positions": _dev(mesh2[0]), "indices": _dev(mesh2[1])}
    out = tm.compute_metrics(m1, m2, metrics, radii, 1000, seed=3)
    _same(out.numpy(), want)


def test_metrics_of_upstreams_cubes(gold):
    g = gold["metrics"]
    mesh1 = orc.unit_cube()
    mesh2 = orc.unit_cube(g["scale"])
    metrics = [orc.pm.METRIC_CODES[m] for m in g["metrics"]]
    st, got, _ = abi_metrics(mesh1, mesh2, metrics, g["fscore_radius"],
                             g["n_sampled_points"])
    assert st == OK
    print("cube metrics:", got)
    np.testing.assert_allclose(got, np.array(g["values"]), rtol=g["rtol"])


def test_metrics_errors_leave_the_values_alone():
    mesh1, mesh2 = soup(20, seed=16), soup(20, seed=17)
    flat = (mesh2[0], np.zeros_like(mesh2[1]))  # total area 0
    bad = (mesh2[0].copy(), mesh2[1])
    bad[0][3, 0] = np.nan
    far = (mesh2[0], mesh2[1].copy())
    far[1][2, 2] = 1000
    for second in (flat, bad, far, (mesh2[0], mesh2[1][:0])):
        st, values, raw = abi_metrics(mesh1, second, [CHAMFER, FSCORE],
                                      [0.1], 50)
        assert st == INVALID_ARG
        assert (values == POISON).all() and raw["counts"] == [[-7], [-7]]
    st, values, _ = abi_metrics(mesh1, mesh2, [CHAMFER, FSCORE], [], 50)
    assert st == INVALID_ARG and (values == POISON).all()
    st, values, _ = abi_metrics(mesh1, mesh2, [CHAMFER, 5], [0.1], 50)
    assert st == INVALID_ARG
    st, values, _ = abi_metrics(mesh1, mesh2, [CHAMFER], [0.1], 0)
    assert st == INVALID_ARG and (values == POISON).all()
    st, values, _ = abi_metrics(mesh1, mesh2, [CHAMFER, HAUSDORFF], [], 50,
                                capacity=1)
    assert st == 3 and (values == POISON).all()  # O3DMI_ERR_CAPACITY
    f64 = (mesh1[0].astype(np.float64), mesh1[1])
    st, values, _ = abi_metrics(f64, f64, [CHAMFER], [], 50)
    assert st == UNSUPPORTED and (values == POISON).all()
