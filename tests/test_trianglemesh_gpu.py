"""GPU tests of the TriangleMesh operators against the numpy restatement
(tests/_trianglemesh_oracle.py) and upstream's literal vectors
(tests/golden/trianglemesh_vectors.json). Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _trianglemesh_oracle as orc

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, CAPACITY = 0, 1, 3
F32, F64, I32, I64 = 0, 1, 4, 5
FLOATS = [np.float32, np.float64]
INTS = [np.int32, np.int64]
CODE = {np.float32: F32, np.float64: F64, np.int32: I32, np.int64: I64}
TCODE = {torch.float32: F32, torch.float64: F64, torch.int32: I32,
         torch.int64: I64}
POISON = -777.0
MAX_TRIANGLES = 1 << 29  # kMeshMaxTriangles (csrc/trianglemesh.h)


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
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want))


def _mesh_args(p, t):
    L = _L()
    return (L.ptr(p), p.shape[0], TCODE[p.dtype], L.ptr(t), t.shape[0],
            TCODE[t.dtype])


def _index_args(t, v):
    return (_L().ptr(t), t.shape[0], TCODE[t.dtype], v)


def _poison(shape, dtype):
    return torch.full(shape, POISON, dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def gold():
    return orc.golden()


def random_mesh(v, m, fdt, idt, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    p = (scale * rng.standard_normal((v, 3))).astype(fdt)
    t = rng.integers(0, v, (m, 3)).astype(idt)
    return p, t


# ---- the ABI calls, outputs poisoned first -----------------------------------------
def abi_triangle_normals(p, t):
    pd, td = _dev(p), _dev(t)
    out = _poison((len(t), 3), pd.dtype)
    st = _L().lib().o3dmi_trianglemesh_compute_triangle_normals(
        *_mesh_args(pd, td), _L().ptr(out), None)
    return st, out.cpu().numpy()


def abi_triangle_areas(p, t):
    pd, td = _dev(p), _dev(t)
    out = _poison((len(t),), pd.dtype)
    st = _L().lib().o3dmi_trianglemesh_compute_triangle_areas(
        *_mesh_args(pd, td), _L().ptr(out), None)
    return st, out.cpu().numpy()


def abi_surface_area(p, t):
    pd, td = _dev(p), _dev(t)
    area = C.c_double(POISON)
    st = _L().lib().o3dmi_trianglemesh_surface_area(
        *_mesh_args(pd, td), C.byref(area), None)
    return st, area.value


def abi_normalize(n):
    nd = _dev(n)
    st = _L().lib().o3dmi_trianglemesh_normalize_normals(
        _L().ptr(nd), len(n), CODE[n.dtype.type], None)
    return st, nd.cpu().numpy()


def abi_vertex_normal_sum(t, tn, v):
    td, nd = _dev(t), _dev(tn)
    out = _poison((v, 3), nd.dtype)
    st = _L().lib().o3dmi_trianglemesh_compute_vertex_normals(
        _L().ptr(td), len(t), CODE[t.dtype.type], _L().ptr(nd),
        CODE[tn.dtype.type], v, _L().ptr(out), None)
    return st, out.cpu().numpy()


def abi_vertex_normals(p, t, normalized):
    pd, td = _dev(p), _dev(t)
    tn = _poison((len(t), 3), pd.dtype)
    vn = _poison((len(p), 3), pd.dtype)
    st = _L().lib().o3dmi_trianglemesh_vertex_normals(
        *_mesh_args(pd, td), _L().ptr(tn), _L().ptr(vn), int(normalized), None)
    return st, tn.cpu().numpy(), vn.cpu().numpy()


def abi_edges(t, v, allow_boundary, capacity):
    td = _dev(t)
    out = torch.full((max(capacity, 0), 2), -9, dtype=td.dtype, device="cuda")
    n = C.c_int64(-5)
    st = _L().lib().o3dmi_trianglemesh_get_non_manifold_edges(
        *_index_args(td, v), int(allow_boundary),
        _L().ptr(out) if capacity > 0 else None, capacity, C.byref(n), None)
    return st, n.value, out.cpu().numpy()


def abi_cluster(p, t, capacity=None, per_cluster=True):
    pd, td = _dev(p), _dev(t)
    m = len(t)
    capacity = m if capacity is None else capacity
    labels = torch.full((m,), -9, dtype=torch.int32, device="cuda")
    counts = torch.full((max(capacity, 1),), -9, dtype=torch.int64,
                        device="cuda")
    areas = _poison((max(capacity, 1),), torch.float64)
    n = C.c_int64(-5)
    st = _L().lib().o3dmi_trianglemesh_cluster_connected_triangles(
        *_mesh_args(pd, td), _L().ptr(labels), C.byref(n),
        _L().ptr(counts) if per_cluster else None,
        _L().ptr(areas) if per_cluster else None, capacity, None)
    return (st, n.value, labels.cpu().numpy(), counts.cpu().numpy(),
            areas.cpu().numpy())


def abi_select_faces(t, v, mask):
    td, md = _dev(t), _dev(np.asarray(mask, np.uint8))
    vmask = torch.full((v,), 9, dtype=torch.uint8, device="cuda")
    out = torch.full_like(td, -9)
    nt, nv = C.c_int64(-5), C.c_int64(-5)
    st = _L().lib().o3dmi_trianglemesh_select_faces_by_mask(
        *_index_args(td, v), _L().ptr(md), _L().ptr(vmask), _L().ptr(out),
        C.byref(nt), C.byref(nv), None)
    return st, nt.value, nv.value, vmask.cpu().numpy(), out.cpu().numpy()


def abi_select_index(t, v, indices):
    td, idx = _dev(t), _dev(np.asarray(indices, np.int64))
    vmask = torch.full((v,), 9, dtype=torch.uint8, device="cuda")
    tmask = torch.full((len(t),), 9, dtype=torch.uint8, device="cuda")
    out = torch.full_like(td, -9)
    nt, nv, ni = C.c_int64(-5), C.c_int64(-5), C.c_int64(-5)
    st = _L().lib().o3dmi_trianglemesh_select_by_index(
        *_index_args(td, v), _L().ptr(idx), len(indices), _L().ptr(vmask),
        _L().ptr(tmask), _L().ptr(out), C.byref(nt), C.byref(nv),
        C.byref(ni), None)
    return (st, nt.value, nv.value, ni.value, vmask.cpu().numpy(),
            tmask.cpu().numpy(), out.cpu().numpy())


def abi_remove_unreferenced(t, v):
    td = _dev(t)
    vmask = torch.full((v,), 9, dtype=torch.uint8, device="cuda")
    out = torch.full_like(td, -9)
    nv = C.c_int64(-5)
    st = _L().lib().o3dmi_trianglemesh_remove_unreferenced_vertices(
        *_index_args(td, v), _L().ptr(vmask), _L().ptr(out), C.byref(nv),
        None)
    return st, nv.value, vmask.cpu().numpy(), out.cpu().numpy()


# ---- elementwise ---------------------------------------------------------------------
@pytest.mark.parametrize("idt", INTS)
@pytest.mark.parametrize("fdt", FLOATS)
@pytest.mark.parametrize("m", [1, 63, 64, 65, 5000])
def test_triangle_normals_areas_and_surface(m, fdt, idt):
    p, t = random_mesh(max(3, m // 2), m, fdt, idt, seed=m)
    st, n = abi_triangle_normals(p, t)
    assert st == OK
    _same(n, orc.triangle_normals(p, t))
    st, a = abi_triangle_areas(p, t)
    assert st == OK
    _same(a, orc.triangle_areas(p, t))
    st, area = abi_surface_area(p, t)
    assert st == OK and area == orc.tree_sum(a)


@pytest.mark.parametrize("fdt", FLOATS)
def test_degenerate_and_overflowing_triangles(fdt):
    p = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [1e19, 0, 0],
                  [0, 1e19, 0], [-1e19, 1e19, 3e18]], fdt)
    # collinear, a repeated vertex, three times one vertex, and (Float32) a
    # cross product whose squares overflow
    t = np.array([[0, 1, 2], [0, 0, 3], [3, 3, 3], [4, 5, 6], [0, 4, 5]],
                 np.int32)
    st, n = abi_triangle_normals(p, t)
    assert st == OK
    _same(n, orc.triangle_normals(p, t))
    st, a = abi_triangle_areas(p, t)
    assert st == OK
    want = orc.triangle_areas(p, t)
    _same(a, want)
    assert a[:3].tolist() == [0.0, 0.0, 0.0]
    assert np.isinf(want[3]) == (fdt is np.float32)


@pytest.mark.parametrize("fdt", FLOATS)
def test_normalize_normals_is_the_mesh_rule(fdt):
    tiny = np.finfo(fdt).tiny
    rng = np.random.default_rng(3)
    special = np.array([[np.nan, 1, 2], [3, np.nan, 4], [5, 6, np.nan],
                        [0, 0, 0], [-0.0, 0, 0],
                        [tiny / 8, 0, 0],            # squares underflow to 0
                        [tiny * 2 ** 40, tiny * 2 ** 41, 0],
                        [np.sqrt(tiny) / 4, np.sqrt(tiny) / 8, 0],
                        [np.inf, 1, 1], [3, 4, 0]], fdt)
    n = np.concatenate([special,
                        rng.standard_normal((300, 3)).astype(fdt)])
    st, got = abi_normalize(n)
    assert st == OK
    _same(got, orc.normalize_normals(n))
    _same(got[0], n[0])  # x is NaN: not stored to (not (0, 0, 1))
    _same(got[1], n[1])  # only y is NaN: stored as it is


# ---- vertex normals ------------------------------------------------------------------
def _mixed_normals(m, fdt, seed):
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-3, 3, (m, 1))
    return (mag * rng.standard_normal((m, 3))).astype(fdt)


def _fan(valence):
    """`valence` triangles around vertex 0; vertex 1 is unreferenced."""
    k = np.arange(valence)
    return np.stack([np.zeros_like(k), 2 + k, 3 + k], 1), valence + 3


@pytest.mark.parametrize("idt", INTS)
@pytest.mark.parametrize("fdt", FLOATS)
@pytest.mark.parametrize("valence", [1, 2, 63, 64, 65, 1000])
def test_vertex_normal_sum_of_a_fan(valence, fdt, idt):
    t, v = _fan(valence)
    t = t.astype(idt)
    tn = _mixed_normals(len(t), fdt, valence)
    st, got = abi_vertex_normal_sum(t, tn, v)
    assert st == OK
    _same(got, orc.vertex_normals(t, tn, v))
    assert _bits(got[1]).tolist() == [0, 0, 0]  # unreferenced: +0


@pytest.mark.parametrize("fdt", FLOATS)
def test_vertex_normal_sum_counts_a_repeated_vertex(fdt):
    t = np.array([[0, 0, 1], [2, 2, 2], [0, 1, 2], [3, 0, 3]], np.int32)
    tn = _mixed_normals(4, fdt, 11)
    st, got = abi_vertex_normal_sum(t, tn, 5)
    assert st == OK
    _same(got, orc.vertex_normals(t, tn, 5))
    _same(got[2], ((tn[1] + tn[1]) + tn[1]) + tn[2])


@pytest.mark.parametrize("idt", INTS)
@pytest.mark.parametrize("fdt", FLOATS)
def test_vertex_normals_of_a_random_mesh(fdt, idt):
    p, t = random_mesh(1000, 5000, fdt, idt, seed=5)
    tn = _mixed_normals(5000, fdt, 6)
    st, got = abi_vertex_normal_sum(t, tn, 1000)
    assert st == OK
    _same(got, orc.vertex_normals(t, tn, 1000))
    st, again = abi_vertex_normal_sum(t, tn, 1000)
    _same(again, got)  # the same bits on every run
    # the public chain: triangle normals, the sum, the mesh normalisation
    for normalized in (False, True):
        st, tri_n, vn = abi_vertex_normals(p, t, normalized)
        assert st == OK
        want_tn = orc.triangle_normals(p, t)
        _same(tri_n, want_tn)
        want = orc.vertex_normals(t, want_tn, 1000)
        _same(vn, orc.normalize_normals(want) if normalized else want)


@pytest.mark.parametrize("fdt", FLOATS)
def test_vertex_normals_without_triangles(fdt):
    t = np.zeros((0, 3), np.int32)
    st, got = abi_vertex_normal_sum(t, np.zeros((0, 3), fdt), 7)
    assert st == OK and _bits(got).tolist() == [[0, 0, 0]] * 7
    st, _, vn = abi_vertex_normals(np.ones((7, 3), fdt), t, True)
    assert st == OK and _bits(vn).tolist() == [[0, 0, 0]] * 7


# ---- non-manifold edges --------------------------------------------------------------
def _edges(t, v, allow_boundary):
    st, n, _ = abi_edges(t, v, allow_boundary, -1)
    assert st == OK
    st, n2, out = abi_edges(t, v, allow_boundary, n)
    assert st == OK and n2 == n
    return out


BOX = [[4, 7, 5], [4, 6, 7], [0, 2, 4], [2, 6, 4], [0, 1, 2], [1, 3, 2],
       [1, 5, 7], [1, 7, 3], [2, 3, 7], [2, 7, 6], [0, 4, 1], [1, 4, 5]]


@pytest.mark.parametrize("idt", INTS)
def test_non_manifold_edges_golden(gold, idt):
    g = gold["non_manifold"]
    t = np.array(g["triangles"], idt)
    closed = _edges(t, 9, False)
    assert closed.dtype == idt
    assert closed.tolist() == orc.non_manifold_edges(t, False).tolist()
    assert sorted(map(tuple, closed.tolist())) == \
        sorted(map(tuple, g["edges_no_boundary"]))
    boundary = _edges(t, 9, True)
    assert boundary.tolist() == orc.non_manifold_edges(t, True).tolist()
    assert set(map(tuple, boundary.tolist())) == \
        set(map(tuple, g["edges_no_boundary"])) - \
        set(map(tuple, g["multiplicity_one"]))


@pytest.mark.parametrize("idt", INTS)
def test_non_manifold_edges_small_cases(idt):
    box = np.array(BOX, idt)
    for allow in (False, True):
        assert _edges(box, 8, allow).shape == (0, 2)  # closed: none
    one = np.array([[2, 0, 1]], idt)
    assert _edges(one, 3, True).shape == (0, 2)
    assert _edges(one, 3, False).tolist() == [[0, 1], [0, 2], [1, 2]]
    # an edge shared by 5 triangles
    fan = np.array([[0, 1, 2 + k] for k in range(5)], idt)
    assert _edges(fan, 7, True).tolist() == [[0, 1]]
    assert _edges(fan, 7, False).tolist() == \
        orc.non_manifold_edges(fan, False).tolist()
    # duplicate triangles: every edge of the pair has multiplicity 2 + 2
    dup = np.array(BOX + BOX[:2], idt)
    assert _edges(dup, 8, True).tolist() == \
        orc.non_manifold_edges(dup, True).tolist()
    assert len(_edges(dup, 8, True)) == 5


def test_non_manifold_edges_random_and_capacity():
    _, t = random_mesh(300, 5000, np.float32, np.int32, seed=9)
    for allow in (False, True):
        assert _edges(t, 300, allow).tolist() == \
            orc.non_manifold_edges(t, allow).tolist()
    want = orc.non_manifold_edges(t, True)
    st, n, _ = abi_edges(t, 300, True, -1)  # counting mode
    assert st == OK and n == len(want)
    st, n, out = abi_edges(t, 300, True, len(want) - 1)
    assert st == CAPACITY and n == len(want)
    assert (out == -9).all()  # nothing written
    st, n, _ = abi_edges(np.zeros((0, 3), np.int32), 5, True, -1)
    assert st == OK and n == 0


# ---- clustering ----------------------------------------------------------------------
def _strip(n, first_vertex=0):
    """n triangles of a strip: triangle k is (k, k + 1, k + 2)."""
    k = np.arange(n) + first_vertex
    return np.stack([k, k + 1, k + 2], 1)


def _check_cluster(p, t):
    st, n, labels, counts, areas = abi_cluster(p, t)
    assert st == OK
    want = orc.cluster_connected_triangles(p, t)
    assert n == len(want[1])
    assert labels.tolist() == want[0].tolist()
    assert counts[:n].tolist() == want[1].tolist()
    _same(areas[:n], want[2])
    return labels, counts[:n], areas[:n]


@pytest.mark.parametrize("idt", INTS)
@pytest.mark.parametrize("fdt", FLOATS)
@pytest.mark.parametrize("name", ["cluster_boxes", "cluster_pairs"])
def test_cluster_goldens(gold, name, fdt, idt):
    g = gold[name]
    p = np.array(g["vertices"], fdt)
    labels, counts, areas = _check_cluster(p, np.array(g["triangles"], idt))
    assert labels.tolist() == g["labels"]
    assert counts.tolist() == g["n_triangles"]
    # Float64 positions: upstream's literals exactly; Float32: the literals
    # rounded to float32 and widened
    assert areas.tolist() == np.array(g["areas"], fdt).astype(np.float64) \
        .tolist()


@pytest.mark.parametrize("idt", INTS)
def test_cluster_labels_follow_the_lowest_triangle_index(idt):
    rng = np.random.default_rng(2)
    p = rng.standard_normal((10010, 3)).astype(np.float32)
    strip = _strip(5000).astype(idt)
    labels, counts, _ = _check_cluster(p, strip)
    assert counts.tolist() == [5000] and not labels.any()
    labels, counts, _ = _check_cluster(p, strip[rng.permutation(5000)])
    assert counts.tolist() == [5000]
    # two strips interleaved in index: even triangles one, odd the other
    two = np.empty((5000, 3), idt)
    two[0::2] = _strip(2500)
    two[1::2] = _strip(2500, first_vertex=5000)
    labels, counts, _ = _check_cluster(p, two)
    assert counts.tolist() == [2500, 2500]
    assert labels.tolist() == [0, 1] * 2500
    # the second strip first: it is cluster 0 now
    labels, _, _ = _check_cluster(p, two[::-1].copy())
    assert labels.tolist() == [0, 1] * 2500


def test_cluster_adjacency_is_by_edge():
    p = np.random.default_rng(4).standard_normal((8, 3))
    bow_tie = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    labels, counts, _ = _check_cluster(p, bow_tie)
    assert labels.tolist() == [0, 1] and counts.tolist() == [1, 1]
    # adjacent only through the degenerate edge (5, 5), as upstream
    degenerate = np.array([[5, 5, 0], [5, 5, 1]], np.int32)
    labels, counts, _ = _check_cluster(p, degenerate)
    assert labels.tolist() == [0, 0] and counts.tolist() == [2]
    singles = (3 * np.arange(300)[:, None] + np.arange(3)).astype(np.int32)
    p = np.random.default_rng(5).standard_normal((900, 3)).astype(np.float32)
    labels, counts, _ = _check_cluster(p, singles)
    assert labels.tolist() == list(range(300)) and (counts == 1).all()


@pytest.mark.parametrize("fdt", FLOATS)
def test_cluster_area_runs(fdt):
    """Clusters of 511, 512, 513 and 1025 triangles with random areas: the run
    boundaries of the two-level sum, with the members interleaved in index."""
    sizes = [511, 512, 513, 1025]
    rng = np.random.default_rng(8)
    tris, first = [], 0
    for n in sizes:
        tris.append(_strip(n, first))
        first += n + 2
    order = rng.permutation(sum(sizes))
    t = np.concatenate(tris)[order].astype(np.int32)
    scale = 10.0 ** rng.uniform(-3, 3, (first, 1))
    p = (scale * rng.standard_normal((first, 3))).astype(fdt)
    _, counts, areas = _check_cluster(p, t)
    assert sorted(counts.tolist()) == sizes
    # and the sum is a sum: numpy's pairwise one agrees to rounding
    want = orc.cluster_connected_triangles(p, t)
    per_tri = np.array([orc.legacy_triangle_area(p, r) for r in t])
    plain = [per_tri[want[0] == c].sum() for c in range(4)]
    assert np.allclose(areas, plain, rtol=1e-12)


def test_cluster_capacity_and_empty():
    p, t = random_mesh(600, 400, np.float32, np.int32, seed=12)
    want = orc.cluster_connected_triangles(p, t)
    c = len(want[1])
    assert c > 2
    st, n, labels, counts, areas = abi_cluster(p, t, capacity=-1)
    assert st == OK and n == c  # counting mode: nothing written
    assert (labels == -9).all() and (counts == -9).all()
    st, n, labels, counts, areas = abi_cluster(p, t, capacity=c - 1)
    assert st == CAPACITY and n == c
    assert (labels == -9).all() and (counts == -9).all() and \
        (areas == POISON).all()
    st, n, labels, counts, areas = abi_cluster(p, t, capacity=c,
                                               per_cluster=False)
    assert st == OK and labels.tolist() == want[0].tolist()
    st, n, _, _, _ = abi_cluster(p, np.zeros((0, 3), np.int32))
    assert st == OK and n == 0


# ---- selection -----------------------------------------------------------------------
@pytest.mark.parametrize("idt", INTS)
def test_select_faces_by_mask(gold, idt):
    box, g = gold["box"], gold["select_faces_by_mask"]
    t = np.array(box["triangles"], idt)
    st, nt, nv, vmask, out = abi_select_faces(t, 8, g["mask"])
    assert st == OK and (nt, nv) == (2, 4)
    assert out[:nt].tolist() == g["expected"]["triangles"]
    assert np.array(box["vertices"])[vmask.astype(bool)].tolist() == \
        np.array(g["expected"]["vertices"], float).tolist()
    _, t = random_mesh(700, 3000, np.float32, idt, seed=21)
    rng = np.random.default_rng(22)
    for mask in (np.zeros(3000, np.uint8), np.ones(3000, np.uint8),
                 (rng.random(3000) < 0.05).astype(np.uint8)):
        st, nt, nv, vmask, out = abi_select_faces(t, 700, mask)
        want_v, want_t = orc.select_faces_by_mask(t, 700, mask)
        assert st == OK and nt == len(want_t) and nv == want_v.sum()
        assert vmask.tolist() == want_v.astype(int).tolist()
        assert out[:nt].tolist() == want_t.tolist()
        assert (out[nt:] == -9).all()


@pytest.mark.parametrize("idt", INTS)
def test_select_by_index(gold, idt):
    box = gold["box"]
    t = np.array(box["triangles"], idt)
    for case in ("basic", "duplicate", "negative", "no_triangles"):
        g = gold["select_by_index"][case]
        st, nt, nv, ni, vmask, tmask, out = abi_select_index(t, 8,
                                                             g["indices"])
        assert st == OK and ni == g.get("ignored", 0), case
        assert out[:nt].tolist() == g["expected"]["triangles"], case
        assert np.array(box["vertices"])[vmask.astype(bool)].tolist() == \
            np.array(g["expected"]["vertices"], float).tolist(), case
        assert nv == len(g["expected"]["vertices"])
    _, t = random_mesh(200, 3000, np.float32, idt, seed=23)
    rng = np.random.default_rng(24)
    indices = np.concatenate([rng.integers(0, 200, 150), [-1, 200, -2 ** 40,
                                                          2 ** 40, 7, 7]])
    st, nt, nv, ni, vmask, tmask, out = abi_select_index(t, 200, indices)
    want_v, want_m, want_t, ignored = orc.select_by_index(t, 200, indices)
    assert st == OK and ni == ignored == 4 and nv == want_v.sum()
    assert nt == len(want_t) > 0
    assert vmask.tolist() == want_v.astype(int).tolist()
    assert tmask.tolist() == want_m.astype(int).tolist()
    assert out[:nt].tolist() == want_t.tolist()


@pytest.mark.parametrize("idt", INTS)
def test_remove_unreferenced_vertices(gold, idt):
    g = gold["remove_unreferenced_vertices"]
    t = np.array(g["triangles"], idt)
    st, nv, vmask, out = abi_remove_unreferenced(t, len(g["vertices"]))
    assert st == OK and nv == 18
    assert vmask.tolist() == g["vertex_mask"]
    assert out.tolist() == g["expected_triangles"]
    # the first and the last vertex unreferenced
    t = (1 + _strip(40)).astype(idt)
    st, nv, vmask, out = abi_remove_unreferenced(t, 44)
    assert st == OK and nv == 42
    assert vmask.tolist() == [0] + [1] * 42 + [0]
    assert out.tolist() == _strip(40).tolist()


def test_python_mirror_copies_attributes(gold):
    tm = _tm()
    box = gold["box"]
    mesh = {"positions": _dev(np.array(box["vertices"], np.float32)),
            "indices": _dev(np.array(box["triangles"], np.int64)),
            "colors": _dev((np.arange(24).reshape(8, 3) * 10)
                           .astype(np.uint8)),
            "labels": _dev(np.array(box["vertex_labels"], np.float32)),
            "triangle_labels": _dev(np.array(box["triangle_labels"],
                                             np.float32))}
    want = gold["select_faces_by_mask"]["expected"]
    mask = _dev(np.array(gold["select_faces_by_mask"]["mask"], bool))
    by_index = _dev(np.array([2, 2, -4, 3, 6, 7, 99], np.int64))
    for out in (tm.select_faces_by_mask(mesh, mask),
                tm.select_by_index(mesh, by_index)):
        assert out["positions"].cpu().tolist() == want["vertices"]
        assert out["indices"].cpu().tolist() == want["triangles"]
        assert out["indices"].dtype == torch.int64
        assert out["labels"].cpu().tolist() == want["vertex_labels"]
        assert out["triangle_labels"].cpu().tolist() == \
            want["triangle_labels"]
        assert out["colors"].dtype == torch.uint8
        assert out["colors"].cpu().tolist() == \
            [[10 * (3 * u + c) for c in range(3)] for u in (2, 3, 6, 7)]
    bare = tm.select_by_index(mesh, by_index, copy_attributes=False)
    assert sorted(bare) == ["indices", "positions"]
    none = tm.select_by_index(mesh, _dev(np.array([0, 3, 4], np.int64)))
    assert "indices" not in none and "triangle_labels" not in none
    assert none["positions"].cpu().tolist() == \
        gold["select_by_index"]["no_triangles"]["expected"]["vertices"]
    assert tm.select_by_index(mesh, _dev(np.zeros(0, np.int64))) == {}
    empty = tm.select_faces_by_mask(mesh, torch.zeros_like(mask))
    assert empty["positions"].shape == (0, 3)
    assert empty["indices"].shape == (0, 3)
    no_tris = {"positions": mesh["positions"]}
    assert tm.compute_triangle_areas(
        {**no_tris, "indices": mesh["indices"][:0]})["triangle_areas"] \
        .shape == (0,)
    assert tm.get_surface_area(no_tris) == 0.0
    assert tm.remove_unreferenced_vertices(no_tris)["positions"].shape == \
        (0, 3)
    assert tm.get_surface_area(mesh) == 6.0
    assert tm.get_non_manifold_edges(mesh).shape == (0, 2)
    labels, counts, areas = tm.cluster_connected_triangles(mesh)
    assert counts.cpu().tolist() == [12] and areas.cpu().tolist() == [6.0]
    assert not labels.any()


# ---- errors --------------------------------------------------------------------------
@pytest.mark.parametrize("idt", INTS)
@pytest.mark.parametrize("bad_index", [-1, 8])
def test_out_of_range_triangle_index_writes_nothing(gold, bad_index, idt):
    box = gold["box"]
    p = np.array(box["vertices"], np.float32)
    t = np.array(box["triangles"], idt)
    t[7, 1] = bad_index
    st, n = abi_triangle_normals(p, t)
    assert st == INVALID_ARG and (n == POISON).all()
    st, a = abi_triangle_areas(p, t)
    assert st == INVALID_ARG and (a == POISON).all()
    st, area = abi_surface_area(p, t)
    assert st == INVALID_ARG and area == POISON
    st, vn = abi_vertex_normal_sum(t, np.ones((12, 3), np.float32), 8)
    assert st == INVALID_ARG and (vn == POISON).all()
    st, tn, vn = abi_vertex_normals(p, t, True)
    assert st == INVALID_ARG and (tn == POISON).all() and (vn == POISON).all()
    st, n, out = abi_edges(t, 8, True, 40)
    assert st == INVALID_ARG and n == -5 and (out == -9).all()
    st, n, labels, counts, areas = abi_cluster(p, t)
    assert st == INVALID_ARG and n == -5 and (labels == -9).all()
    assert (counts == -9).all() and (areas == POISON).all()
    st, nt, nv, vmask, out = abi_select_faces(t, 8, np.ones(12, np.uint8))
    assert st == INVALID_ARG and (vmask == 9).all() and (out == -9).all()
    st, nt, nv, ni, vmask, tmask, out = abi_select_index(t, 8, [1, 2])
    assert st == INVALID_ARG and (vmask == 9).all() and (tmask == 9).all()
    assert (out == -9).all()
    st, nv, vmask, out = abi_remove_unreferenced(t, 8)
    assert st == INVALID_ARG and (vmask == 9).all() and (out == -9).all()


def test_null_arguments_and_limits():
    L = _L()
    lib = L.lib()
    p = _dev(np.zeros((4, 3), np.float32))
    t = _dev(np.array([[0, 1, 2]], np.int32))
    out = _poison((4, 3), torch.float32)
    n = C.c_int64(0)
    P, T, O = L.ptr(p), L.ptr(t), L.ptr(out)
    f = lib.o3dmi_trianglemesh_compute_triangle_normals
    for args in ((None, 4, F32, T, 1, I32, O), (P, 4, F32, None, 1, I32, O),
                 (P, 4, F32, T, 1, I32, None), (P, 4, I32, T, 1, I32, O),
                 (P, 4, F32, T, 1, F32, O), (P, -1, F32, T, 1, I32, O),
                 (P, 1 << 31, F32, T, 1, I32, O), (P, 4, F32, T, -1, I32, O),
                 # m above the limit: refused on the argument alone
                 (P, 4, F32, T, MAX_TRIANGLES + 1, I32, O)):
        assert f(*args, None) == INVALID_ARG, args
    assert lib.o3dmi_trianglemesh_compute_triangle_areas(
        P, 4, F32, T, MAX_TRIANGLES + 1, I32, O, None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_surface_area(
        P, 4, F32, T, 1, I32, None, None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_normalize_normals(
        None, 4, F32, None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_normalize_normals(
        O, 4, I32, None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_compute_vertex_normals(
        T, 1, I32, None, F32, 4, O, None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_compute_vertex_normals(
        T, MAX_TRIANGLES + 1, I32, O, F32, 4, O, None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_vertex_normals(
        P, 4, F32, T, 1, I32, None, None, 1, None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_get_non_manifold_edges(
        T, 1, I32, 4, 1, None, -1, None, None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_get_non_manifold_edges(
        T, 1, I32, 4, 1, None, 5, C.byref(n), None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_get_non_manifold_edges(
        T, MAX_TRIANGLES + 1, I32, 4, 1, None, -1, C.byref(n),
        None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_cluster_connected_triangles(
        P, 4, F32, T, 1, I32, None, C.byref(n), None, None, 1,
        None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_cluster_connected_triangles(
        None, 4, F32, T, 1, I32, O, C.byref(n), None, O, 1,
        None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_cluster_connected_triangles(
        P, 4, F32, T, MAX_TRIANGLES + 1, I32, O, C.byref(n), None, None, 1,
        None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_select_faces_by_mask(
        T, 1, I32, 4, None, O, O, C.byref(n), C.byref(n),
        None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_select_by_index(
        T, 1, I32, 4, None, 2, O, O, O, C.byref(n), C.byref(n), C.byref(n),
        None) == INVALID_ARG
    assert lib.o3dmi_trianglemesh_remove_unreferenced_vertices(
        T, 1, I32, 4, None, O, C.byref(n), None) == INVALID_ARG
    assert (out.cpu().numpy() == POISON).all()


# ---- end to end ----------------------------------------------------------------------
def test_extracted_mesh_end_to_end(tmp_path):
    from test_mesh_gpu import _sphere_grid
    tm = _tm()
    g = _sphere_grid(tmp_path, 8, np.uint16, True)
    mesh = g.extract_triangle_mesh(weight_threshold=3.0)
    p = mesh["positions"].cpu().numpy()
    t = mesh["indices"].cpu().numpy()
    assert len(t) > 500
    labels, counts, areas = tm.cluster_connected_triangles(mesh)
    want = orc.cluster_connected_triangles(p, t)
    assert labels.cpu().tolist() == want[0].tolist()
    assert counts.cpu().tolist() == want[1].tolist()
    _same(areas.cpu().numpy(), want[2])
    largest = int(np.argmax(want[1]))
    kept = tm.select_faces_by_mask(mesh, labels == largest)
    want_v, want_t = orc.select_faces_by_mask(t, len(p), want[0] == largest)
    assert kept["indices"].cpu().tolist() == want_t.tolist()
    _same(kept["positions"].cpu().numpy(), p[want_v])
    _same(kept["normals"].cpu().numpy(),
          mesh["normals"].cpu().numpy()[want_v])
    _same(kept["colors"].cpu().numpy(), mesh["colors"].cpu().numpy()[want_v])
    out = tm.compute_vertex_normals(kept, normalized=True)
    tn = orc.triangle_normals(p[want_v], want_t)
    vn = orc.normalize_normals(orc.vertex_normals(want_t, tn, want_v.sum()))
    _same(out["normals"].cpu().numpy(), vn)
    _same(out["triangle_normals"].cpu().numpy(), orc.normalize_normals(tn))
    # the recomputed normals point the way the extraction's own normals do
    extracted = kept["normals"].cpu().numpy()
    finite = np.isfinite(extracted).all(axis=1)
    assert finite.sum() > 100
    dots = (vn[finite].astype(np.float64) *
            extracted[finite].astype(np.float64)).sum(axis=1)
    assert (dots > 0).all()
