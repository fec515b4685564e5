"""GPU tests of ClipPlane / SlicePlane against the literal restatement
(tests/_trianglemesh_clip_oracle.py). Every comparison with the oracle is bit
for bit (positions, attributes, indices, sources, t); every output is poisoned
before the call."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import _trianglemesh_clip_oracle as orc
import _trianglemesh_subdivide_oracle as sub
from test_trianglemesh_clip_cpu import BOX_P, BOX_T, QUAD_P, QUAD_T, TETRA_P, \
    TETRA_T, _loops

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, CAPACITY, UNSUPPORTED = 0, 1, 3, 7
F32, F64, I32, I64 = 0, 1, 4, 5
CODE = {np.float32: F32, np.float64: F64, np.int32: I32, np.int64: I64}
POISON = -777.0
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                    "open3d_amd", "csrc")


def _constant(path, name):
    text = open(os.path.join(CSRC, path)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


# the workgroup of the clip kernels (trianglemesh_clip.h: kClipBlock = kBlock)
# and the tile of the prefix sums they feed (scan.hip)
assert "constexpr int kClipBlock = kBlock;" in open(
    os.path.join(CSRC, "trianglemesh_clip.h")).read()
CLIP_BLOCK = _constant("common.h", "kBlock")
SCAN_TILE = _constant("scan.hip", "kScanBlock") * \
    _constant("scan.hip", "kScanItems")


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
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want))


def _poison(shape, np_dtype):
    dtype = torch.from_numpy(np.zeros(0, np_dtype)).dtype
    fill = POISON if dtype.is_floating_point else int(POISON)
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def _poisoned(t):
    return t is None or bool((t == POISON).all())


def _p(t):
    return _L().ptr(t)


def _vec(x):
    return (C.c_double * 3)(*[float(e) for e in x])


# ---- the meshes -----------------------------------------------------------------------
def grid(n):
    """The open n x n vertex grid, two triangles a cell."""
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).ravel()
    return np.concatenate([np.stack([a, a + 1, a + n], axis=1),
                           np.stack([a + 1, a + n + 1, a + n], axis=1)])


def _grid_positions(n, seed, exact_diagonal):
    """Vertex (i, j) at (i, j, 0) plus jitter; with exact_diagonal the
    vertices (i, i) keep their small integer coordinates."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    p = np.stack([i.ravel(), j.ravel(), np.zeros(n * n)], axis=1).astype(
        np.float64)
    jitter = 0.3 * rng.standard_normal(p.shape)
    if exact_diagonal:
        jitter[(i == j).ravel()] = 0
    return p + jitter


def _grid_first(m):
    """The first m triangles of the 66 x 66 grid (8450 triangles), whose
    triangles are shuffled so that any prefix crosses the plane."""
    t = grid(66)
    t = t[np.random.default_rng(3).permutation(len(t))]
    return _grid_positions(66, 66, False), t[:m]


def _tetra3():
    p, _, _, t = sub.subdivide_midpoint(TETRA_P, TETRA_T, 3)
    return p, t.astype(np.int64)


ODD_P = np.array([[1, 0, 0], [-1, 0, 0], [1, 1, 0], [-1, 1, 0], [0, 0, 0],
                  [0, 1, 0], [5, 6, 7], [2, 0, 1], [-2, 0, 1], [0, 0, 1]],
                 np.float64)
# degenerate across and inside, doubled, touching with a vertex / an edge from
# below and from above, in the plane, a cut through a vertex; vertex 6 is
# unreferenced
ODD_T = np.array([[0, 0, 1], [0, 1, 1], [0, 0, 2], [0, 0, 0], [0, 1, 2],
                  [0, 1, 2], [4, 1, 3], [4, 5, 3], [4, 5, 0], [4, 5, 9],
                  [4, 7, 8], [5, 8, 7], [3, 2, 1], [9, 4, 2]], np.int64)

EDGE_SIZES = [CLIP_BLOCK - 1, CLIP_BLOCK, CLIP_BLOCK + 1, SCAN_TILE - 1,
              SCAN_TILE, SCAN_TILE + 1]
MESHES = {
    "box": lambda: (BOX_P, BOX_T),
    "quad": lambda: (QUAD_P, QUAD_T),
    "odd": lambda: (ODD_P, ODD_T),
    "tetra3": _tetra3,
    "empty": lambda: (np.zeros((0, 3)), np.zeros((0, 3), np.int64)),
    "no_triangles": lambda: (QUAD_P, np.zeros((0, 3), np.int64)),
    "grid70": lambda: (_grid_positions(70, 70, True), grid(70)),
}
for _m in EDGE_SIZES:
    MESHES["grid66_first_%d" % _m] = functools.partial(_grid_first, _m)

GENERIC = ((0.23, 0.19, 0.31), (0.3, -0.5, 0.8))
# name -> (mesh, point, normal)
PLANES = {
    "box_half": ("box", (0.5, 0, 0), (1, 0, 0)),
    "box_face_1": ("box", (1, 0, 0), (1, 0, 0)),
    "box_face_0": ("box", (0, 0, 0), (-1, 0, 0)),
    "box_whole": ("box", (0, 0, 0), (1, 1, 0)),
    "box_corner": ("box", (0, 0, 0), (-1, -1, -1)),
    "box_face_slice_0": ("box", (0, 0, 0), (1, 0, 0)),
    "box_diagonal": ("box", (0, 0, 0), (1, -1, 0)),
    "box_upstream_slice": ("box", (0, 0.5, 0), (1, 1, 1)),
    "quad": ("quad", (1, 0, 0), (1, 0, 0)),
    "odd": ("odd", (0, 0, 0), (1, 0, 0)),
    "tetra3": ("tetra3",) + GENERIC,
    "tetra3_flipped": ("tetra3", GENERIC[0], tuple(-x for x in GENERIC[1])),
    "empty": ("empty",) + GENERIC,
    "no_triangles": ("no_triangles",) + GENERIC,
    # through the diagonal vertices (i, i, 0), exactly
    "grid70": ("grid70", (35, 35, 0), (1, -1, 2)),
}
for _m in EDGE_SIZES:
    PLANES["grid66_first_%d" % _m] = ("grid66_first_%d" % _m, (32.3, 31.9, 0),
                                      (0.7, -0.4, 0.2))
SMALL = [k for k in sorted(PLANES) if not k.startswith("grid")]
CONTOURS = {"box_upstream_slice": (-0.1, 0, 0.1), "grid70": (0.0, 3.0, -2.0)}


@functools.lru_cache(maxsize=None)
def mesh(name, fdt=np.float64):
    """-> positions, normals, colours (of fdt), triangles (int64)."""
    p, t = MESHES[name]()
    rng = np.random.default_rng(len(name) + 7 * len(p))
    n = rng.standard_normal((len(p), 3)).astype(fdt)
    c = rng.random((len(p), 3)).astype(fdt)
    return p.astype(fdt), n, c, np.asarray(t, np.int64).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def clip_oracle(plane, fdt=np.float64, attrs=True):
    name, point, normal = PLANES[plane]
    p, n, c, t = mesh(name, fdt)
    return orc.clip_plane(p, t, point, normal, normals=n if attrs else None,
                          colors=c if attrs else None)


@functools.lru_cache(maxsize=None)
def slice_oracle(plane, values=(0.0,), fdt=np.float64, attrs=True):
    name, point, normal = PLANES[plane]
    p, n, c, t = mesh(name, fdt)
    return orc.slice_plane(p, t, point, normal, values,
                           normals=n if attrs else None,
                           colors=c if attrs else None)


# ---- the two calls ----------------------------------------------------------------------
def _head(p, n, c, t, point, normal, attr_code):
    ins = [_dev(p), _dev(n), _dev(c), _dev(t)]
    attr_code = CODE[p.dtype.type] if attr_code is None else attr_code
    return ins, (_p(ins[0]), len(p), CODE[p.dtype.type], _p(ins[1]),
                 _p(ins[2]), attr_code, _p(ins[3]), len(t),
                 CODE[t.dtype.type], _vec(point), _vec(normal))


def clip_abi(p, n, c, t, point, normal, capacity=None, optional=True,
             attr_code=None):
    """One call with poisoned outputs of capacity = (vertex rows, triangle
    rows) (None: the count call's answer) -> status, outputs, n_v, n_t."""
    ins, head = _head(p, n, c, t, point, normal, attr_code)
    call = _L().lib().o3dmi_trianglemesh_clip_plane
    n_v, n_t = C.c_int64(-5), C.c_int64(-5)
    if capacity is None:
        st = call(*head, None, None, None, -1, None, 0, None, None, None,
                  C.byref(n_v), C.byref(n_t), None)
        assert st == OK, _L().lib().o3dmi_last_error()
        capacity = (n_v.value, n_t.value)
        n_v, n_t = C.c_int64(-5), C.c_int64(-5)
    vcap, tcap = capacity
    rows = vcap if vcap >= 0 else 8  # a count call: the rows stay untouched
    fdt, idt = p.dtype.type, t.dtype.type
    out = {"positions": _poison((rows, 3), fdt),
           "normals": None if n is None else _poison((rows, 3), fdt),
           "colors": None if c is None else _poison((rows, 3), fdt),
           "triangles": _poison((tcap, 3), idt),
           "triangle_source": _poison((tcap,), idt) if optional else None,
           "vertex_source": _poison((rows, 2), idt) if optional else None,
           "vertex_t": _poison((rows,), np.float64) if optional else None}
    st = call(*head, _p(out["positions"]), _p(out["normals"]),
              _p(out["colors"]), vcap, _p(out["triangles"]), tcap,
              _p(out["triangle_source"]), _p(out["vertex_source"]),
              _p(out["vertex_t"]), C.byref(n_v), C.byref(n_t), None)
    return st, out, n_v.value, n_t.value


def slice_abi(p, n, c, t, point, normal, values, capacity=None, optional=True,
              attr_code=None):
    ins, head = _head(p, n, c, t, point, normal, attr_code)
    k = len(values)
    head += ((C.c_double * max(k, 1))(*[float(x) for x in values]), k)
    call = _L().lib().o3dmi_trianglemesh_slice_plane
    n_p, n_l = C.c_int64(-5), C.c_int64(-5)
    if capacity is None:
        st = call(*head, None, None, None, -1, None, 0, None, None, None,
                  None, C.byref(n_p), C.byref(n_l), None)
        assert st == OK, _L().lib().o3dmi_last_error()
        capacity = (n_p.value, n_l.value)
        n_p, n_l = C.c_int64(-5), C.c_int64(-5)
    pcap, lcap = capacity
    rows = pcap if pcap >= 0 else 8  # a count call: the rows stay untouched
    fdt, idt = p.dtype.type, t.dtype.type
    out = {"positions": _poison((rows, 3), fdt),
           "normals": None if n is None else _poison((rows, 3), fdt),
           "colors": None if c is None else _poison((rows, 3), fdt),
           "lines": _poison((lcap, 2), idt),
           "line_triangle": _poison((lcap,), idt) if optional else None,
           "line_contour": _poison((lcap,), np.int32) if optional else None,
           "point_source": _poison((rows, 2), idt) if optional else None,
           "point_t": _poison((rows,), np.float64) if optional else None}
    st = call(*head, _p(out["positions"]), _p(out["normals"]),
              _p(out["colors"]), pcap, _p(out["lines"]), lcap,
              _p(out["line_triangle"]), _p(out["line_contour"]),
              _p(out["point_source"]), _p(out["point_t"]), C.byref(n_p),
              C.byref(n_l), None)
    return st, out, n_p.value, n_l.value


VERTEX_ROWS = ("positions", "normals", "colors", "vertex_source", "vertex_t",
               "point_source", "point_t")
INDEX_ROWS = ("triangles", "triangle_source", "vertex_source", "lines",
              "line_triangle", "point_source")


def _compare(out, want, n_rows, n_cells, idt, attrs, optional):
    """Every output against the oracle, bit for bit, and poison behind."""
    for name, got in out.items():
        ref = want[name]
        if name in ("normals", "colors") and not attrs:
            assert got is None
            continue
        if got is None:
            assert not optional
            continue
        if name in INDEX_ROWS:
            ref = ref.astype(idt)
        rows = n_rows if name in VERTEX_ROWS else n_cells
        assert len(ref) == rows
        _same(got[:rows].cpu().numpy(), ref)
        assert _poisoned(got[rows:])


def check_clip(plane, fdt=np.float64, idt=np.int32, attrs=True, optional=True,
               slack=0):
    name, point, normal = PLANES[plane]
    p, n, c, t = mesh(name, fdt)
    if not attrs:
        n = c = None
    want = clip_oracle(plane, fdt, attrs)
    capacity = None if slack == 0 else (len(want["positions"]) + slack,
                                        len(want["triangles"]) + slack)
    st, out, n_v, n_t = clip_abi(p, n, c, t.astype(idt), point, normal,
                                 capacity, optional)
    assert st == OK, _L().lib().o3dmi_last_error()
    assert (n_v, n_t) == (len(want["positions"]), len(want["triangles"]))
    _compare(out, want, n_v, n_t, idt, attrs, optional)
    return want


def check_slice(plane, values=(0.0,), fdt=np.float64, idt=np.int32,
                attrs=True, optional=True, slack=0):
    name, point, normal = PLANES[plane]
    p, n, c, t = mesh(name, fdt)
    if not attrs:
        n = c = None
    want = slice_oracle(plane, tuple(values), fdt, attrs)
    capacity = None if slack == 0 else (len(want["positions"]) + slack,
                                        len(want["lines"]) + slack)
    st, out, n_p, n_l = slice_abi(p, n, c, t.astype(idt), point, normal,
                                  values, capacity, optional)
    assert st == OK, _L().lib().o3dmi_last_error()
    assert (n_p, n_l) == (len(want["positions"]), len(want["lines"]))
    _compare(out, want, n_p, n_l, idt, attrs, optional)
    return want


# ---- against the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("plane", SMALL)
def test_clip_every_small_case_matches_the_oracle(plane):
    check_clip(plane)
    check_clip(plane, slack=3)


@pytest.mark.parametrize("plane", SMALL)
def test_slice_every_small_case_matches_the_oracle(plane):
    check_slice(plane, CONTOURS.get(plane, (0.0,)))
    check_slice(plane, slack=3)


def test_the_box_counts_are_upstreams():
    want = check_clip("box_half")
    assert (len(want["positions"]), len(want["triangles"])) == (12, 14)
    want = check_slice("box_upstream_slice", (-0.1, 0, 0.1))
    assert (len(want["positions"]), len(want["lines"])) == (9, 9)
    for plane, counts in (("box_face_1", (4, 2)), ("box_face_0", (4, 2)),
                          ("box_whole", (8, 12)), ("box_corner", (0, 0))):
        want = check_clip(plane)
        assert (len(want["positions"]), len(want["triangles"])) == counts
    for plane, counts in (("box_face_1", (4, 4)), ("box_face_slice_0", (0, 0)),
                          ("box_diagonal", (5, 5))):
        want = check_slice(plane)
        assert (len(want["positions"]), len(want["lines"])) == counts
        assert len(_loops(want["lines"])) == (1 if counts[0] else 0)


@pytest.mark.parametrize("optional", [True, False])
@pytest.mark.parametrize("attrs", [True, False])
@pytest.mark.parametrize("idt", [np.int32, np.int64])
@pytest.mark.parametrize("fdt", [np.float32, np.float64])
def test_every_dtype_with_and_without_attributes(fdt, idt, attrs, optional):
    for plane in ("box_half", "odd", "tetra3", "box_diagonal"):
        check_clip(plane, fdt, idt, attrs, optional)
        check_slice(plane, CONTOURS.get(plane, (0.0, 0.05)), fdt, idt, attrs,
                    optional)


@pytest.mark.parametrize("m", EDGE_SIZES)
def test_launch_edges(m):
    """Triangle counts one below, at and one above the workgroup of the clip
    kernels (kClipBlock = kBlock) and the tile of the prefix sums (kScanBlock
    * kScanItems)."""
    assert EDGE_SIZES == [255, 256, 257, 8191, 8192, 8193]
    want = check_clip("grid66_first_%d" % m, np.float32)
    assert 0 < len(want["triangles"]) and (want["vertex_t"] != 0).any()
    want = check_slice("grid66_first_%d" % m, (0.0, 1.5), np.float32)
    assert len(want["lines"]) > 0


@pytest.mark.parametrize("fdt", [np.float32, np.float64])
def test_grid70_with_a_plane_through_vertices(fdt):
    name, point, normal = PLANES["grid70"]
    p, _, _, t = mesh(name, fdt)
    assert len(t) == 9522
    s = orc.signed_values(p, point, normal)
    assert (s == 0).sum() == 70  # the diagonal, exactly on the plane
    want = check_clip("grid70", fdt, np.int64)
    assert (want["vertex_t"] != 0).sum() > 50
    want = check_slice("grid70", CONTOURS["grid70"], fdt, np.int32)
    vertex_points = want["point_source"][:, 0] == want["point_source"][:, 1]
    assert vertex_points.sum() >= 60 and (~vertex_points).sum() > 50


@pytest.mark.parametrize("values", [(), (0.0,), (0.05, 1e9, 0.05), (-1e9,)])
def test_slice_contour_lists(values):
    """K = 0, 1 and 3 with a repeated value and values outside the mesh's
    range: contours do not share points, an empty contour adds nothing."""
    want = check_slice("tetra3", values)
    one = slice_oracle("tetra3", (0.05,))
    if values == (0.05, 1e9, 0.05):
        assert len(want["positions"]) == 2 * len(one["positions"]) > 0
        assert set(want["line_contour"].tolist()) == {0, 2}
    if values in ((), (-1e9,)):
        assert len(want["positions"]) == 0 and len(want["lines"]) == 0


def test_slice_edge_points_have_clips_bits_on_the_device():
    name, point, normal = PLANES["tetra3"]
    p, n, c, t = mesh(name, np.float32)
    _, clip, n_v, _ = clip_abi(p, n, c, t, point, normal)
    _, cut, n_p, _ = slice_abi(p, n, c, t, point, normal, (0.0,))
    src = clip["vertex_source"].cpu().numpy()
    by_edge = {tuple(e): i for i, e in enumerate(src)}
    rows = [by_edge[tuple(e)] for e in cut["point_source"].cpu().numpy()]
    assert n_p > 8 and len(rows) == n_p
    for name in ("positions", "normals", "colors", ):
        _same(cut[name].cpu().numpy(), clip[name].cpu().numpy()[rows])
    _same(cut["point_t"].cpu().numpy(), clip["vertex_t"].cpu().numpy()[rows])


# ---- the protocol -------------------------------------------------------------------------
def test_count_call_touches_nothing_and_short_capacities_are_refused():
    name, point, normal = PLANES["tetra3"]
    p, n, c, t = mesh(name)
    want = clip_oracle("tetra3")
    n_v, n_t = len(want["positions"]), len(want["triangles"])
    for capacity in ((n_v - 1, n_t), (n_v, n_t - 1), (0, 0)):
        st, out, got_v, got_t = clip_abi(p, n, c, t, point, normal, capacity)
        assert (st, got_v, got_t) == (CAPACITY, n_v, n_t)
        assert all(_poisoned(o) for o in out.values())
    st, out, got_v, got_t = clip_abi(p, n, c, t, point, normal, (n_v, n_t))
    assert (st, got_v, got_t) == (OK, n_v, n_t)
    # a count call (capacity < 0) with outputs given leaves them alone
    st, out, got_v, got_t = clip_abi(p, n, c, t, point, normal, (-1, n_t))
    assert (st, got_v, got_t) == (OK, n_v, n_t)
    assert all(_poisoned(o) for o in out.values())

    values = (0.0, 0.05)
    want = slice_oracle("tetra3", values)
    n_p, n_l = len(want["positions"]), len(want["lines"])
    for capacity in ((n_p - 1, n_l), (n_p, n_l - 1), (0, 0)):
        st, out, got_p, got_l = slice_abi(p, n, c, t, point, normal, values,
                                          capacity)
        assert (st, got_p, got_l) == (CAPACITY, n_p, n_l)
        assert all(_poisoned(o) for o in out.values())
    st, out, got_p, got_l = slice_abi(p, n, c, t, point, normal, values,
                                      (n_p, n_l))
    assert (st, got_p, got_l) == (OK, n_p, n_l)
    st, out, got_p, got_l = slice_abi(p, n, c, t, point, normal, values,
                                      (-1, n_l))
    assert (st, got_p, got_l) == (OK, n_p, n_l)
    assert all(_poisoned(o) for o in out.values())


def _refused(status, p, n, c, t, point=GENERIC[0], normal=GENERIC[1],
             values=(0.0,), attr_code=None, which=("clip", "slice")):
    rows = (len(p) + 3 * len(t), 2 * len(t) + 1)
    if "clip" in which:
        st, out, n_v, n_t = clip_abi(p, n, c, t, point, normal, rows,
                                     attr_code=attr_code)
        assert (st, n_v, n_t) == (status, -5, -5)
        assert all(_poisoned(o) for o in out.values())
    if "slice" in which:
        st, out, n_p, n_l = slice_abi(p, n, c, t, point, normal, values, rows,
                                      attr_code=attr_code)
        assert (st, n_p, n_l) == (status, -5, -5)
        assert all(_poisoned(o) for o in out.values())


def test_refusals_leave_the_outputs_poisoned():
    p, n, c, t = mesh("odd")
    bad = t.copy()
    bad[3, 1] = len(p)
    _refused(INVALID_ARG, p, n, c, bad)
    bad[3, 1] = -1
    _refused(INVALID_ARG, p, n, c, bad)
    for row in (0, 6):  # referenced, unreferenced
        q = p.copy()
        q[row, 1] = np.nan
        _refused(INVALID_ARG, q, n, c, t)
    q = c.copy()
    q[6, 2] = np.nan
    _refused(INVALID_ARG, p, n, q, t)
    q = n.copy()
    q[2, 0] = np.inf
    _refused(INVALID_ARG, p, q, c, t)
    _refused(INVALID_ARG, p, n, c, t, normal=(0, 0, 0))
    _refused(INVALID_ARG, p, n, c, t, normal=(0, np.nan, 1))
    _refused(INVALID_ARG, p, n, c, t, point=(np.inf, 0, 0))
    _refused(INVALID_ARG, p, n, c, t, values=(0.0, np.inf), which=("slice",))
    _refused(INVALID_ARG, p, n, c, t, values=(np.nan,), which=("slice",))
    # finite inputs whose signed value overflows
    _refused(INVALID_ARG, p * 1e200, n, c, t, normal=(1e200, 0, 0))
    _refused(UNSUPPORTED, p, n.astype(np.float32), c.astype(np.float32), t,
             attr_code=F32)


def test_size_limits_are_checked_before_any_access():
    L = _L().lib()
    at, nrm = _vec(GENERIC[0]), _vec(GENERIC[1])
    n_a, n_b = C.c_int64(-5), C.c_int64(-5)

    def clip(v, m):
        return L.o3dmi_trianglemesh_clip_plane(
            None, v, F32, None, None, F32, None, m, I32, at, nrm, None, None,
            None, -1, None, 0, None, None, None, C.byref(n_a), C.byref(n_b),
            None)

    def cut(v, m, k):
        return L.o3dmi_trianglemesh_slice_plane(
            None, v, F32, None, None, F32, None, m, I32, at, nrm,
            (C.c_double * k)(), k, None, None, None, -1, None, 0, None, None,
            None, None, C.byref(n_a), C.byref(n_b), None)

    assert clip(10, 2 ** 28 + 1) == INVALID_ARG
    assert clip(2 ** 31 - 3 * 2 ** 20, 2 ** 20) == INVALID_ARG
    assert cut(10, 2 ** 29 + 1, 1) == INVALID_ARG
    assert cut(10, 2 ** 26 + 1, 8) == INVALID_ARG
    assert cut(2 ** 31 - 3 * 2 ** 20, 2 ** 20, 1) == INVALID_ARG
    assert (n_a.value, n_b.value) == (-5, -5)
    # at the limits the sizes pass and the null positions are what is refused
    assert clip(10, 2 ** 28) == INVALID_ARG
    assert b"null" in L.o3dmi_last_error()
    assert cut(10, 2 ** 26, 8) == INVALID_ARG
    assert b"null" in L.o3dmi_last_error()


def test_the_same_call_twice_gives_identical_bytes():
    name, point, normal = PLANES["grid70"]
    p, n, c, t = mesh(name, np.float32)
    a = clip_abi(p, n, c, t, point, normal)
    b = clip_abi(p, n, c, t, point, normal)
    assert a[2:] == b[2:]
    for k in a[1]:
        assert torch.equal(a[1][k].view(torch.uint8), b[1][k].view(torch.uint8))
    a = slice_abi(p, n, c, t, point, normal, CONTOURS["grid70"])
    b = slice_abi(p, n, c, t, point, normal, CONTOURS["grid70"])
    assert a[2:] == b[2:]
    for k in a[1]:
        assert torch.equal(a[1][k].view(torch.uint8), b[1][k].view(torch.uint8))


# ---- the Python layer ---------------------------------------------------------------------
def _mesh_dict(name, fdt=np.float32, idt=np.int32):
    p, n, c, t = mesh(name, fdt)
    rng = np.random.default_rng(9)
    extra = rng.standard_normal((len(p), 2, 2)).astype(np.float32)
    tn = rng.standard_normal((len(t), 3)).astype(fdt)
    return {"positions": _dev(p), "normals": _dev(n), "colors": _dev(c),
            "indices": _dev(t.astype(idt)), "weights": _dev(extra),
            "triangle_normals": _dev(tn)}, extra, tn


def test_python_clip_plane_carries_every_attribute():
    tm = _tm()
    m, extra, tn = _mesh_dict("tetra3")
    _, point, normal = PLANES["tetra3"]
    want = clip_oracle("tetra3", np.float32)
    for at, nrm in ((point, normal),
                    (torch.tensor(point, dtype=torch.float64),
                     torch.tensor(normal, dtype=torch.float64).cuda())):
        out = tm.clip_plane(m, at, nrm)
        for name in ("positions", "normals", "colors"):
            _same(out[name].cpu().numpy(), want[name])
        _same(out["indices"].cpu().numpy(),
              want["triangles"].astype(np.int32))
        _same(out["weights"].cpu().numpy(),
              orc.interpolate(extra, want["vertex_source"], want["vertex_t"]))
        _same(out["triangle_normals"].cpu().numpy(),
              tn[want["triangle_source"]])
        assert set(out) == set(m)
    # integer points and normals are taken as they are
    out = tm.clip_plane({"positions": _dev(BOX_P), "indices": _dev(BOX_T)},
                        torch.tensor([1, 0, 0]), [1, 0, 0])
    _same(out["positions"].cpu().numpy(), BOX_P[[1, 3, 5, 7]])


def test_python_slice_plane_returns_a_line_set():
    tm = _tm()
    m, extra, _ = _mesh_dict("tetra3")
    _, point, normal = PLANES["tetra3"]
    values = (0.0, 0.05)
    want = slice_oracle("tetra3", values, np.float32)
    out = tm.slice_plane(m, point, normal, values)
    for name in ("positions", "normals", "colors"):
        _same(out[name].cpu().numpy(), want[name])
    _same(out["indices"].cpu().numpy(), want["lines"].astype(np.int32))
    _same(out["line_triangle"].cpu().numpy(),
          want["line_triangle"].astype(np.int32))
    _same(out["line_contour"].cpu().numpy(), want["line_contour"])
    _same(out["weights"].cpu().numpy(),
          orc.interpolate(extra, want["point_source"], want["point_t"]))
    assert "triangle_normals" not in out
    default = tm.slice_plane(m, point, normal)
    _same(default["positions"].cpu().numpy(),
          slice_oracle("tetra3", (0.0,), np.float32)["positions"])


def test_python_refuses_an_integer_vertex_attribute():
    tm = _tm()
    m, _, _ = _mesh_dict("box")
    m["labels"] = torch.zeros(8, dtype=torch.int32, device="cuda")
    for call in (tm.clip_plane, tm.slice_plane):
        with pytest.raises(ValueError, match="labels"):
            call(m, (0.5, 0, 0), (1, 0, 0))
    with pytest.raises(ValueError, match="shape"):
        tm.clip_plane({"positions": m["positions"]}, (0, 0), (1, 0, 0))


def test_python_clip_output_is_a_mesh_the_other_calls_take():
    tm = _tm()
    p, _, _, t = mesh("tetra3")
    m = {"positions": _dev(p), "indices": _dev(t)}
    _, point, normal = PLANES["tetra3"]
    above = tm.clip_plane(m, point, normal)
    below = tm.clip_plane(m, point, [-x for x in normal])
    assert tm.is_edge_manifold(above) and tm.is_edge_manifold(below)
    assert not tm.is_edge_manifold(above, allow_boundary_edges=False)
    total = tm.get_surface_area(m)
    parts = tm.get_surface_area(above) + tm.get_surface_area(below)
    assert abs(parts - total) <= 1e-10 * total
