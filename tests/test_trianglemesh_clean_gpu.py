"""GPU tests of the mesh clean-up calls, the CSR adjacency, the smoothing
filters and the vertex clustering against the numpy restatement
(tests/_trianglemesh_clean_oracle.py). Every comparison with the oracle is bit
for bit; every output is poisoned before the call."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _trianglemesh_clean_oracle as orc

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, CAPACITY, UNSUPPORTED = 0, 1, 3, 7
F32, F64, I32, I64 = 0, 1, 4, 5
FLOATS = [np.float32, np.float64]
INTS = [np.int32, np.int64]
CODE = {np.float32: F32, np.float64: F64, np.int32: I32, np.int64: I64}
POISON = -777.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _L():
    from open3d_amd import _lib
    return _lib


def _tm():
    from open3d_amd import trianglemesh
    return trianglemesh


def _dev(a):
    return None if a is None else \
        torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want))


def _poison(shape, like):
    dtype = like if isinstance(like, torch.dtype) else \
        torch.from_numpy(np.zeros(0, like)).dtype
    fill = POISON if dtype.is_floating_point else int(POISON)
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def _poisoned(t):
    return bool((t == POISON).all())


def _code(a):
    return CODE[a.dtype.type]


def _p(t):
    return _L().ptr(t)


def random_mesh(v, m, fdt, idt, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((v, 3)).astype(fdt),
            rng.integers(0, v, (m, 3)).astype(idt))


def fan(hub, first_rim, rim):
    """rim - 1 triangles around `hub` over the rim vertices first_rim ..."""
    r = np.arange(first_rim, first_rim + rim)
    return np.stack([np.full(rim - 1, hub), r[:-1], r[1:]], axis=1)


# ---- the ABI calls, outputs poisoned first -----------------------------------------
def abi_dup_vertices(p, t):
    pd, td = _dev(p), _dev(t)
    vmask = torch.full((len(p),), 7, dtype=torch.uint8, device="cuda")
    tris = _poison(t.shape, t.dtype.type)
    n = C.c_int64(-5)
    st = _L().lib().o3dmi_trianglemesh_remove_duplicated_vertices(
        _p(pd), len(p), _code(p), _p(td), len(t), _code(t), _p(vmask),
        _p(tris), C.byref(n), None)
    return st, vmask.cpu().numpy(), tris.cpu().numpy(), n.value


def abi_remove_triangles(which, t, v):
    td = _dev(t)
    tmask = torch.full((len(t),), 7, dtype=torch.uint8, device="cuda")
    tris = _poison(t.shape, t.dtype.type)
    n = C.c_int64(-5)
    call = getattr(_L().lib(), "o3dmi_trianglemesh_remove_%s_triangles" % which)
    st = call(_p(td), len(t), _code(t), v, _p(tmask), _p(tris), C.byref(n),
              None)
    return st, tmask.cpu().numpy(), tris.cpu().numpy(), n.value


def abi_adjacency(t, v, capacity):
    td = _dev(t)
    splits = torch.full((v + 1,), -9, dtype=torch.int64, device="cuda")
    nbrs = _poison((max(capacity, 1),), t.dtype.type)
    n = C.c_int64(-5)
    st = _L().lib().o3dmi_trianglemesh_compute_adjacency_list(
        _p(td), len(t), _code(t), v, _p(splits), _p(nbrs), capacity,
        C.byref(n), None)
    return st, splits.cpu().numpy(), nbrs.cpu().numpy(), n.value


FILTERS = {
    "sharpen": "o3dmi_trianglemesh_filter_sharpen",
    "simple": "o3dmi_trianglemesh_filter_smooth_simple",
    "laplacian": "o3dmi_trianglemesh_filter_smooth_laplacian",
    "taubin": "o3dmi_trianglemesh_filter_smooth_taubin",
}


def abi_filter(kind, p, n, c, t, iterations, factors, scope, attr_code=None):
    ins = [_dev(p), _dev(n), _dev(c)]
    td = _dev(t)
    outs = [None if a is None else _poison(a.shape, a.dtype)
            for a in ins]
    attr_code = _code(p) if attr_code is None else attr_code
    st = getattr(_L().lib(), FILTERS[kind])(
        _p(ins[0]), len(p), _code(p), _p(ins[1]), _p(ins[2]), attr_code,
        _p(td), len(t), _code(t), iterations, *[float(f) for f in factors],
        scope, _p(outs[0]), _p(outs[1]), _p(outs[2]), None)
    return st, outs


def abi_cluster(p, n, c, t, voxel_size, contraction):
    ins = [_dev(p), _dev(n), _dev(c)]
    td = _dev(t)
    outs = [None if a is None else _poison(a.shape, a.dtype)
            for a in ins]
    tris = _poison(t.shape, t.dtype.type)
    nv, nt = C.c_int64(-5), C.c_int64(-5)
    st = _L().lib().o3dmi_trianglemesh_simplify_vertex_clustering(
        _p(ins[0]), len(p), _code(p), _p(ins[1]), _p(ins[2]), _code(p),
        _p(td), len(t), _code(t), float(voxel_size), contraction,
        _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(tris), C.byref(nv),
        C.byref(nt), None)
    return st, outs, tris, nv.value, nt.value


# ---- the representative table: vertices -----------------------------------------------
def check_dup_vertices(p, t):
    st, vmask, tris, n = abi_dup_vertices(p, t)
    assert st == OK
    want_mask, want_tris, want_n = orc.remove_duplicated_vertices(p, t)
    assert n == want_n
    _same(vmask, want_mask)
    _same(tris, want_tris)


@pytest.mark.parametrize("fdt", FLOATS)
@pytest.mark.parametrize("idt", INTS)
def test_duplicated_vertices_small(fdt, idt):
    empty_t = np.zeros((0, 3), idt)
    st, _, _, n = abi_dup_vertices(np.zeros((0, 3), fdt), empty_t)
    assert (st, n) == (OK, 0)
    check_dup_vertices(np.array([[1, 2, 3]], fdt), np.array([[0, 0, 0]], idt))
    # every thread on one slot
    p = np.tile(np.array([[0.5, -1.25, 3.0]], fdt), (3000, 1))
    t = np.random.default_rng(0).integers(0, 3000, (500, 3)).astype(idt)
    check_dup_vertices(p, t)
    st, vmask, tris, n = abi_dup_vertices(p, t)
    assert n == 1 and vmask[0] == 1 and not tris.any()


@pytest.mark.parametrize("fdt", FLOATS)
def test_duplicated_vertices_zeros_and_nans(fdt):
    nan = np.nan
    p = np.array([[0.0, 1, -0.0], [-0.0, 1, 0.0], [nan, 1, 2], [nan, 1, 2],
                  [3, nan, 0], [0.0, 1, 0.0], [3, nan, 0], [7, 7, 7]], fdt)
    t = np.array([[0, 1, 5], [2, 3, 4], [6, 7, 1]], np.int32)
    check_dup_vertices(p, t)
    st, vmask, tris, n = abi_dup_vertices(p, t)
    assert vmask.tolist() == [1, 0, 1, 1, 1, 0, 1, 1] and n == 6
    assert tris.tolist() == [[0, 0, 0], [1, 2, 3], [4, 5, 0]]


@pytest.mark.parametrize("fdt,idt", [(np.float32, np.int64),
                                     (np.float64, np.int32)])
def test_duplicated_vertices_lattice(fdt, idt):
    """~70 000 rows, each lattice point 2-4 times in shuffled order: dense
    collisions, and the scan's and the sort's 8192-row tiles are crossed."""
    rng = np.random.default_rng(3)
    pts = np.stack(np.meshgrid(np.arange(29), np.arange(29), np.arange(28),
                               indexing="ij"), -1).reshape(-1, 3)
    reps = rng.integers(2, 5, len(pts))
    p = np.repeat(pts, reps, axis=0)[rng.permutation(int(reps.sum()))]
    p = (p - 14).astype(fdt)  # zeros included
    t = rng.integers(0, len(p), (9000, 3)).astype(idt)
    assert 60000 < len(p) < 80000
    check_dup_vertices(p, t)


# ---- the representative table: triangles ----------------------------------------------
@pytest.mark.parametrize("idt", INTS)
def test_duplicated_triangles(idt):
    rng = np.random.default_rng(4)
    head = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (5, 5, 3), (5, 3, 5),
            (3, 5, 5), (5, 3, 3), (4, 4, 4), (2, 1, 0), (9, 8, 7)]
    body = rng.integers(0, 40, (20000, 3))  # 64 000 triples: many repeats
    t = np.concatenate([head, body, [(8, 7, 9), (7, 9, 8)]]).astype(idt)
    st, tmask, tris, n = abi_remove_triangles("duplicated", t, 40)
    want_mask, want = orc.remove_duplicated_triangles(t)
    assert st == OK and n == len(want)
    _same(tmask, want_mask)
    _same(tris[:n], want)
    assert _poisoned(torch.from_numpy(tris[n:]))
    assert tmask[:11].tolist() == [1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 1]
    assert tmask[-2:].tolist() == [0, 0]  # (9,8,7) again, 20 000 rows on


@pytest.mark.parametrize("idt", INTS)
def test_degenerate_triangles(idt):
    rng = np.random.default_rng(5)
    t = rng.integers(0, 12, (9001, 3)).astype(idt)
    st, tmask, tris, n = abi_remove_triangles("degenerate", t, 12)
    want_mask, want = orc.remove_degenerate_triangles(t)
    assert st == OK and 0 < n == len(want) < len(t)
    _same(tmask, want_mask)
    _same(tris[:n], want)
    for which in ("degenerate", "duplicated"):
        st, _, _, n = abi_remove_triangles(which, np.zeros((0, 3), idt), 5)
        assert (st, n) == (OK, 0)


# ---- adjacency ---------------------------------------------------------------------------
def fans_mesh(idt):
    """Hubs 0..3 with 63, 64, 65 and 300 rim vertices (the thread / wave edge
    and several 64-blocks), a (6,6,7) triangle, duplicated triangles, one
    isolated vertex (the last)."""
    parts, nxt = [], 4
    for hub, rim in enumerate((63, 64, 65, 300)):
        parts.append(fan(hub, nxt, rim))
        nxt += rim
    parts.append(np.array([[6, 6, 7], [4, 5, 6], [5, 6, 4], [4, 5, 6]]))
    return np.concatenate(parts).astype(idt), nxt + 1


def check_adjacency(t, v):
    st, _, _, n = abi_adjacency(t, v, -1)
    want_splits, want = orc.adjacency_csr(t, v)
    assert st == OK and n == len(want)
    st, splits, nbrs, n = abi_adjacency(t, v, len(want))
    assert st == OK and n == len(want)
    _same(splits, want_splits)
    _same(nbrs[:n], want.astype(t.dtype))
    return splits, nbrs


@pytest.mark.parametrize("idt", INTS)
def test_adjacency_fans(idt):
    t, v = fans_mesh(idt)
    splits, nbrs = check_adjacency(t, v)
    deg = np.diff(splits)
    assert deg[:4].tolist() == [63, 64, 65, 300] and deg[-1] == 0
    assert 6 in nbrs[splits[6]:splits[7]]  # its own neighbour


@pytest.mark.parametrize("idt", INTS)
def test_adjacency_random_and_capacity(idt):
    _, t = random_mesh(500, 2000, np.float32, idt, 6)
    check_adjacency(t, 500)
    want_splits, want = orc.adjacency_csr(t, 500)
    st, splits, nbrs, n = abi_adjacency(t, 500, -1)  # counts only
    assert st == OK and n == len(want)
    assert (splits == -9).all() and _poisoned(torch.from_numpy(nbrs))
    st, splits, nbrs, n = abi_adjacency(t, 500, len(want) - 1)
    assert st == CAPACITY and n == len(want)
    assert (splits == -9).all() and _poisoned(torch.from_numpy(nbrs))
    st, splits, _, n = abi_adjacency(np.zeros((0, 3), idt), 7, 0)
    assert st == OK and n == 0 and not splits.any()


# ---- filters -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden",
                           "trianglemesh_clean_vectors.json")) as f:
        return json.load(f)


def filter_mesh(fdt, idt):
    """v = 2000 + a 300-fan (the wave path) + one isolated vertex."""
    rng = np.random.default_rng(8)
    p, t = random_mesh(2000, 6000, fdt, idt, 7)
    extra = rng.standard_normal((302, 3)).astype(fdt)
    t = np.concatenate([t, fan(2000, 2001, 300).astype(idt)])
    p = np.concatenate([p, extra])
    n = rng.standard_normal(p.shape).astype(fdt)
    c = rng.random(p.shape).astype(fdt)
    return p, n, c, t


KINDS = [("sharpen", [0.3], (1, 2, 3)), ("simple", [], (1, 2, 3)),
         ("laplacian", [0.5], (1, 2, 3)), ("taubin", [0.5, -0.53], (1, 2))]


def check_filter(kind, p, n, c, t, iterations, factors, scope):
    st, outs = abi_filter(kind, p, n, c, t, iterations, factors, scope)
    assert st == OK
    want = orc.run_filter(kind, p, n, c, t, iterations, factors, scope)
    for got, w in zip(outs, want):
        assert (got is None) == (w is None)
        if w is not None:
            _same(got.cpu().numpy(), w)
    return outs


@pytest.mark.parametrize("kind,factors,iters", KINDS,
                         ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("scope", [0, 1, 2, 3])
@pytest.mark.parametrize("fdt,idt", [(np.float32, np.int32),
                                     (np.float64, np.int64)])
def test_filters_equal_the_oracle(kind, factors, iters, scope, fdt, idt):
    p, n, c, t = filter_mesh(fdt, idt)
    for iterations in iters:  # both ping-pong parities
        outs = check_filter(kind, p, n, c, t, iterations, factors, scope)
        got = [o.cpu().numpy() for o in outs]
        for a, (o, given) in enumerate(zip(got, (p, n, c))):
            if scope not in (0, (3, 2, 1)[a]):
                _same(o, given)  # outside the scope: a copy
        _same(got[0][-1], p[-1])  # the isolated vertex


@pytest.mark.parametrize("fdt", FLOATS)
def test_filters_golden_star(gold, fdt):
    t = np.array(gold["star"]["triangles"], np.int32)
    for kind, steps in gold["filters"].items():
        p = np.array(gold["star"]["vertices"], fdt)
        for step in steps:
            outs = check_filter(kind, p, None, None, t, step["iterations"],
                                step["args"], 0)
            p = outs[0].cpu().numpy()
            orc.expect_eq(p, step["expected"], step["threshold"])


def test_filters_without_attributes_or_iterations():
    p, n, c, t = filter_mesh(np.float32, np.int32)
    for kind, factors, _ in KINDS:
        # the scope names attributes the mesh does not have: copies
        check_filter(kind, p, None, c, t, 2, factors, 2)
        check_filter(kind, p, n, None, t, 1, factors, 0)
        for iterations in (0, -3):
            outs = check_filter(kind, p, n, c, t, iterations, factors, 0)
            for o, given in zip(outs, (p, n, c)):
                _same(o.cpu().numpy(), given)
    # no triangles: every vertex is isolated
    outs = check_filter("simple", p, n, c, np.zeros((0, 3), np.int32), 2, [],
                        0)
    _same(outs[0].cpu().numpy(), p)


def test_filters_refuse_bad_arguments():
    p, n, c, t = filter_mesh(np.float64, np.int32)
    L = _L()
    pd, nd, cd, td = _dev(p), _dev(n), _dev(c), _dev(t)
    out = _poison(p.shape, pd.dtype)
    lib = L.lib()

    def sharpen(po, no, co, scope=0, attr=F64):
        return lib.o3dmi_trianglemesh_filter_sharpen(
            _p(pd), len(p), F64, _p(nd), _p(cd), attr, _p(td), len(t), I32, 1,
            1.0, scope, _p(po), _p(no), _p(co), None)

    o2, o3 = torch.empty_like(out), torch.empty_like(out)
    assert sharpen(pd, o2, o3) == INVALID_ARG       # in place
    assert sharpen(out, nd[1:], o3) == INVALID_ARG  # partial overlap
    assert sharpen(out, out, o3) == INVALID_ARG     # two outputs in one
    assert sharpen(out, None, o3) == INVALID_ARG    # normals without output
    assert sharpen(out, o2, o3, scope=4) == INVALID_ARG
    assert sharpen(out, o2, o3, attr=F32) == UNSUPPORTED
    assert _poisoned(out)


# ---- clustering ----------------------------------------------------------------------------
def cluster_mesh(fdt, idt):
    rng = np.random.default_rng(9)
    p, t = random_mesh(3000, 8000, fdt, idt, 10)
    t[:50, 1] = t[:50, 0]  # triangles that name a vertex twice
    n = rng.standard_normal(p.shape).astype(fdt)
    c = rng.random(p.shape).astype(fdt)
    return p, n, c, t


def check_cluster(p, n, c, t, voxel_size, contraction):
    st, outs, tris, nv, nt = abi_cluster(p, n, c, t, voxel_size, contraction)
    assert st == OK
    want = orc.simplify_vertex_clustering(p, n, c, t, voxel_size, contraction)
    assert nv == len(want["positions"]) and nt == len(want["triangles"])
    for got, name in zip(outs, ("positions", "normals", "colors")):
        assert (got is None) == (want[name] is None)
        if got is not None:
            _same(got[:nv].cpu().numpy(), want[name])
            assert _poisoned(got[nv:])
    _same(tris[:nt].cpu().numpy(), want["triangles"])
    assert _poisoned(tris[nt:])
    return want


@pytest.mark.parametrize("contraction", [orc.AVERAGE, orc.QUADRIC])
@pytest.mark.parametrize("fdt,idt", [(np.float32, np.int64),
                                     (np.float64, np.int32)])
def test_clustering_equals_the_oracle(contraction, fdt, idt):
    p, n, c, t = cluster_mesh(fdt, idt)
    largest = []
    for voxel_size in (1e-4, 0.45, 1.0, 8.0):
        want = check_cluster(p, n, c, t, voxel_size, contraction)
        largest.append(np.bincount(want["new_index"]).max())
        # numbered by first occurrence
        first = np.unique(want["new_index"], return_index=True)[1]
        assert (np.diff(first) > 0).all()
    assert largest[0] == 1 and 5 <= largest[1] <= 64
    assert 64 < largest[2] <= 512 and largest[3] > 512
    check_cluster(p, None, None, t, 0.45, contraction)


def test_clustering_triangles():
    """Collapsed triangles leave, equal ones leave but for the first, the
    flipped twin stays."""
    p = np.array([[0, 0, 0], [0.1, 0, 0], [5, 0, 0], [5.1, 0, 0], [0, 5, 0],
                  [0, 5.1, 0], [9, 9, 9]], np.float32)
    t = np.array([[0, 2, 4], [1, 3, 5], [2, 4, 0], [0, 4, 2], [0, 1, 2],
                  [5, 3, 1], [4, 6, 2]], np.int32)
    want = check_cluster(p, None, None, t, 1.0, orc.AVERAGE)
    assert want["new_index"].tolist() == [0, 0, 1, 1, 2, 2, 3]
    assert want["triangles"].tolist() == [[0, 1, 2], [0, 2, 1], [1, 2, 3]]


@pytest.mark.parametrize("fdt", FLOATS)
def test_quadric_cube_corner_is_exact(fdt):
    """Three faces x = 1, y = 2, z = 3 meeting in one voxel, triangle areas
    powers of two: all arithmetic is exact and the vertex is (1, 2, 3)."""
    p = np.array([[1, 2, 3],                      # the corner
                  [1, 2.25, 3], [1, 2, 3.25],     # on x = 1
                  [1.25, 2, 3], [1, 2, 3.25],     # on y = 2
                  [1.25, 2, 3], [1, 2.25, 3],     # on z = 3
                  [1, 66, 3], [1, 2, 35],         # far: other voxels
                  [33, 2, 3], [1, 2, 67],
                  [17, 2, 3], [1, 18, 3]], fdt)
    t = np.array([[0, 7, 8], [0, 10, 9], [0, 11, 12]], np.int32)
    st, outs, tris, nv, nt = abi_cluster(p, None, None, t, 0.75, orc.QUADRIC)
    assert st == OK
    want = orc.simplify_vertex_clustering(p, None, None, t, 0.75, orc.QUADRIC)
    got = outs[0][:nv].cpu().numpy()
    _same(got, want["positions"])
    assert want["new_index"][:7].tolist() == [0] * 7
    assert got[0].tolist() == [1.0, 2.0, 3.0]
    average = orc.simplify_vertex_clustering(p, None, None, t, 0.75,
                                             orc.AVERAGE)
    assert average["positions"][0].tolist() != [1.0, 2.0, 3.0]


def test_quadric_on_a_plane_is_the_average():
    rng = np.random.default_rng(12)
    p = np.zeros((400, 3), np.float64)
    p[:, :2] = rng.random((400, 2)) * 4
    p[:, 2] = 0.5
    t = rng.integers(0, 400, (900, 3)).astype(np.int32)
    st, q_outs, _, nv, _ = abi_cluster(p, None, None, t, 1.0, orc.QUADRIC)
    st2, a_outs, _, nv2, _ = abi_cluster(p, None, None, t, 1.0, orc.AVERAGE)
    assert st == OK and st2 == OK and nv == nv2 > 4
    _same(q_outs[0][:nv].cpu().numpy(), a_outs[0][:nv].cpu().numpy())
    check_cluster(p, None, None, t, 1.0, orc.QUADRIC)


def test_clustering_refuses_bad_voxel_sizes():
    p, n, c, t = cluster_mesh(np.float32, np.int32)
    for voxel_size in (0.0, -1.0, float("nan"), float("inf"), 1e-12):
        # upstream's two refusals, and a size that is not finite
        assert not orc.voxel_size_ok(p, voxel_size) or np.isinf(voxel_size)
        st, outs, tris, nv, nt = abi_cluster(p, n, c, t, voxel_size, 0)
        assert st == INVALID_ARG
        assert all(_poisoned(o) for o in outs) and _poisoned(tris)
    st, outs, _, _, _ = abi_cluster(p, n, c, t, 1.0, 2)
    assert st == INVALID_ARG and _poisoned(outs[0])
    st, _, _, nv, nt = abi_cluster(np.zeros((0, 3), np.float32), None, None,
                                   np.zeros((0, 3), np.int32), 1.0, 0)
    assert (st, nv, nt) == (OK, 0, 0)


# ---- across all calls ----------------------------------------------------------------------
@pytest.mark.parametrize("idt", INTS)
def test_bad_triangle_index_or_position_leaves_outputs_alone(idt):
    p, n, c, t = filter_mesh(np.float32, idt)
    v = len(p)
    for bad in (v, -1):
        tb = t.copy()
        tb[4321, 1] = bad
        st, vmask, tris, _ = abi_dup_vertices(p, tb)
        assert st == INVALID_ARG and (vmask == 7).all()
        assert _poisoned(torch.from_numpy(tris))
        for which in ("duplicated", "degenerate"):
            st, tmask, tris, _ = abi_remove_triangles(which, tb, v)
            assert st == INVALID_ARG and (tmask == 7).all()
            assert _poisoned(torch.from_numpy(tris))
        st, splits, nbrs, _ = abi_adjacency(tb, v, 100000)
        assert st == INVALID_ARG and (splits == -9).all()
        assert _poisoned(torch.from_numpy(nbrs))
        for kind, factors, _ in KINDS:
            st, outs = abi_filter(kind, p, n, c, tb, 1, factors, 0)
            assert st == INVALID_ARG and all(_poisoned(o) for o in outs)
        st, outs, tris, _, _ = abi_cluster(p, n, c, tb, 0.5, 1)
        assert st == INVALID_ARG and _poisoned(tris)
        assert all(_poisoned(o) for o in outs)
    for bad in (np.nan, np.inf):
        pb = p.copy()
        pb[1234, 2] = bad
        for kind, factors, _ in KINDS:
            st, outs = abi_filter(kind, pb, n, c, t, 1, factors, 0)
            assert st == INVALID_ARG and all(_poisoned(o) for o in outs)
        st, outs, tris, _, _ = abi_cluster(pb, n, c, t, 0.5, 0)
        assert st == INVALID_ARG and _poisoned(tris)
        assert all(_poisoned(o) for o in outs)


# ---- the Python mirror -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def box():
    with open(os.path.join(ROOT, "tests", "golden",
                           "trianglemesh_vectors.json")) as f:
        g = json.load(f)["box"]
    p = np.array(g["vertices"], np.float32)
    t = np.array(g["triangles"], np.int64)
    return {"positions": p, "indices": t,
            "colors": np.array(g["vertex_colors"], np.float32),
            "labels": np.array(g["vertex_labels"], np.float32),
            "triangle_labels": np.array(g["triangle_labels"], np.float32)}


def _mesh(box):
    return {k: _dev(v) for k, v in box.items()}


def _host(mesh):
    return {k: v.cpu().numpy() for k, v in mesh.items()}


def test_mirror_clean_up(box):
    tm = _tm()
    p, t = box["positions"], box["indices"]
    doubled = {
        "positions": np.concatenate([p, p]),
        "colors": np.concatenate([box["colors"], box["colors"] + 1]),
        "labels": np.concatenate([box["labels"], box["labels"] + 100]),
        "indices": np.concatenate([t, t[:, [1, 2, 0]] + 8, [[0, 0, 1]]]),
        "triangle_labels": np.concatenate(
            [box["triangle_labels"], box["triangle_labels"] + 50,
             [[99, 99, 99]]]
        ).astype(np.float32),
    }
    out = tm.remove_duplicated_vertices(_mesh(doubled))
    got = _host(out)
    for name in ("positions", "colors", "labels"):  # the first copy's rows
        _same(got[name], box[name])
    assert got["indices"][:12].tolist() == t.tolist()
    out = tm.remove_duplicated_triangles(out)
    got = _host(out)
    assert got["indices"].tolist() == t.tolist() + [[0, 0, 1]]
    assert got["triangle_labels"].tolist() == \
        box["triangle_labels"].tolist() + [[99.0, 99.0, 99.0]]
    got = _host(tm.remove_degenerate_triangles(out))
    assert got["indices"].tolist() == t.tolist()
    _same(got["triangle_labels"], box["triangle_labels"])
    _same(got["positions"], p)
    splits, nbrs = tm.compute_adjacency_list(_mesh(box))
    want_splits, want = orc.adjacency_csr(t, 8)
    _same(splits.cpu().numpy(), want_splits)
    _same(nbrs.cpu().numpy(), want)


def test_mirror_filters_and_clustering(box):
    tm = _tm()
    p, c, t = box["positions"], box["colors"], box["indices"]
    mesh = _mesh(box)
    calls = [
        ("sharpen", [1.0], tm.filter_sharpen(mesh)),
        ("simple", [], tm.filter_smooth_simple(mesh)),
        ("laplacian", [0.5], tm.filter_smooth_laplacian(mesh)),
        ("taubin", [0.5, -0.53], tm.filter_smooth_taubin(mesh)),
        ("taubin", [0.4, -0.5], tm.filter_smooth_taubin(
            mesh, 3, 0.4, -0.5, tm.FilterScope.Color)),
    ]
    for i, (kind, factors, out) in enumerate(calls):
        scope, iterations = (1, 3) if i == 4 else (0, 1)
        want = orc.run_filter(kind, p, None, c, t, iterations, factors, scope)
        got = _host(out)
        _same(got["positions"], want[0])
        _same(got["colors"], want[2])
        _same(got["labels"], box["labels"])
        assert "normals" not in got
        _same(got["indices"], t)
    assert (tm.FilterScope.All, tm.FilterScope.Color, tm.FilterScope.Normal,
            tm.FilterScope.Vertex) == (0, 1, 2, 3)
    with_normals = tm.compute_triangle_normals(mesh)
    for contraction in (tm.SimplificationContraction.Average,
                        tm.SimplificationContraction.Quadric):
        out = _host(tm.simplify_vertex_clustering(with_normals, 1.2,
                                                  contraction))
        want = orc.simplify_vertex_clustering(p, None, c, t, 1.2, contraction)
        _same(out["positions"], want["positions"])
        _same(out["colors"], want["colors"])
        _same(out["indices"], want["triangles"])
        assert "labels" not in out
        assert out["triangle_normals"].shape == (len(want["triangles"]), 3)
    assert tm.simplify_vertex_clustering(mesh, 0.5)["positions"].shape[0] == 8
