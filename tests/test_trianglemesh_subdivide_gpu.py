"""GPU tests of SubdivideMidpoint / SubdivideLoop against the literal
restatement (tests/_trianglemesh_subdivide_oracle.py). Every comparison with
the oracle is bit for bit; every output is poisoned before the call."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _trianglemesh_subdivide_oracle as orc

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, CAPACITY, UNSUPPORTED = 0, 1, 3, 7
F32, F64, I32, I64 = 0, 1, 4, 5
CODE = {np.float32: F32, np.float64: F64, np.int32: I32, np.int64: I64}
POISON = -777.0
CALLS = {"midpoint": "o3dmi_trianglemesh_subdivide_midpoint",
         "loop": "o3dmi_trianglemesh_subdivide_loop"}
ORACLE = {"midpoint": orc.subdivide_midpoint, "loop": orc.subdivide_loop}


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


# ---- the meshes: (number of vertices, triangles) -------------------------------------
def closed_fan(rim):
    """rim triangles around hub 0 over the rim vertices 1 .. rim."""
    r = np.arange(1, rim + 1)
    return np.stack([np.zeros(rim, np.int64), r, np.roll(r, -1)], axis=1)


def grid(n):
    """The open n x n vertex grid, two triangles a cell."""
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).ravel()
    return np.concatenate([np.stack([a, a + 1, a + n], axis=1),
                           np.stack([a + 1, a + n + 1, a + n], axis=1)])


TETRA = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]
MESHES = {
    "triangle": (3, [[0, 1, 2]]),
    "tetra": (4, TETRA),
    "pair_equal_winding": (4, [[0, 1, 2], [3, 2, 1]]),
    "pair_opposite_winding": (4, [[0, 1, 2], [1, 2, 3]]),
    "fan3": (4, closed_fan(3)),     # the |nbs| == 3 branch at the hub
    "fan6": (7, closed_fan(6)),
    "fan70": (71, closed_fan(70)),  # a list beyond kLongCornerList = 64
    "edge70": (72, [[0, 1, 2 + i] for i in range(70)]),  # a long edge run
    # a doubled triangle, (a, a, b), (a, a, a), an unreferenced vertex
    "odd": (7, [[0, 1, 2], [0, 1, 2], [3, 3, 4], [5, 5, 5]]),
    "unreferenced_only": (3, np.zeros((0, 3), np.int64)),
    "empty": (0, np.zeros((0, 3), np.int64)),
    "soup": (50, np.random.default_rng(11).integers(0, 50, (200, 3))),
    "grid33": (33 * 33, grid(33)),
}


@functools.lru_cache(maxsize=None)
def mesh(name, fdt=np.float64):
    """-> positions, normals, colours (of fdt), triangles (int64)."""
    v, t = MESHES[name]
    rng = np.random.default_rng(len(name) + 7 * v)
    p = rng.standard_normal((v, 3)).astype(fdt)
    n = rng.standard_normal((v, 3)).astype(fdt)
    c = rng.random((v, 3)).astype(fdt)
    return p, n, c, np.asarray(t, np.int64).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def oracle(name, which, iterations, fdt=np.float64, attrs=True):
    p, n, c, t = mesh(name, fdt)
    return ORACLE[which](p, t, iterations, normals=n if attrs else None,
                         colors=c if attrs else None)


def abi(which, p, n, c, t, iterations, capacity=None, attr_code=None,
        tri_rows=None):
    """One call with poisoned outputs of `capacity` rows (None: the count
    call's answer) -> status, [positions, normals, colours], triangles, n_v,
    n_t, all as the call left them."""
    ins = [_dev(p), _dev(n), _dev(c)]
    td = _dev(t)
    attr_code = CODE[p.dtype.type] if attr_code is None else attr_code
    call = getattr(_L().lib(), CALLS[which])
    head = (_p(ins[0]), len(p), CODE[p.dtype.type], _p(ins[1]), _p(ins[2]),
            attr_code, _p(td), len(t), CODE[t.dtype.type], iterations)
    n_v, n_t = C.c_int64(-5), C.c_int64(-5)
    if capacity is None:
        st = call(*head, None, None, None, -1, None, C.byref(n_v),
                  C.byref(n_t), None)
        assert st == OK, _L().lib().o3dmi_last_error()
        capacity = n_v.value
    if tri_rows is None:
        tri_rows = len(t) * 4 ** max(iterations, 0)
    outs = [None if a is None else _poison((capacity, 3), p.dtype.type)
            for a in ins]
    tris = _poison((tri_rows, 3), t.dtype.type)
    st = call(*head, _p(outs[0]), _p(outs[1]), _p(outs[2]), capacity, _p(tris),
              C.byref(n_v), C.byref(n_t), None)
    return st, outs, tris, n_v.value, n_t.value


def check_against_oracle(name, which, iterations, fdt=np.float64,
                         idt=np.int32, attrs=True, slack=0):
    p, n, c, t = mesh(name, fdt)
    if not attrs:
        n = c = None
    want = oracle(name, which, iterations, fdt, attrs)
    capacity = None if slack == 0 else len(want[0]) + slack
    st, outs, tris, n_v, n_t = abi(which, p, n, c, t.astype(idt), iterations,
                                   capacity)
    assert st == OK, _L().lib().o3dmi_last_error()
    assert n_v == len(want[0]) and n_t == len(want[3])
    assert n_t == len(t) * 4 ** max(iterations, 0)
    for got, ref in zip(outs, want[:3]):
        assert (got is None) == (ref is None)
        if got is not None:
            _same(got[:n_v].cpu().numpy(), ref)
            assert _poisoned(got[n_v:])  # rows beyond the count stay
    _same(tris.cpu().numpy(), want[3].astype(idt))


# ---- against the oracle ----------------------------------------------------------------
@pytest.mark.parametrize("iterations", [0, 1, 2, 3])
@pytest.mark.parametrize("which", ["midpoint", "loop"])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_every_mesh_matches_the_oracle(name, which, iterations):
    check_against_oracle(name, which, iterations)


@pytest.mark.parametrize("attrs", [True, False])
@pytest.mark.parametrize("idt", [np.int32, np.int64])
@pytest.mark.parametrize("fdt", [np.float32, np.float64])
@pytest.mark.parametrize("which", ["midpoint", "loop"])
def test_every_dtype_with_and_without_attributes(which, fdt, idt, attrs):
    for name, iterations in (("odd", 3), ("soup", 2), ("fan70", 1)):
        check_against_oracle(name, which, iterations, fdt, idt, attrs)


@pytest.mark.parametrize("which", ["midpoint", "loop"])
def test_zero_and_negative_iterations_copy(which):
    p, n, c, t = mesh("soup")
    for iterations in (0, -3):
        st, outs, tris, n_v, n_t = abi(which, p, n, c, t, iterations)
        assert (st, n_v, n_t) == (OK, len(p), len(t))
        for got, ref in zip(outs, (p, n, c)):
            _same(got.cpu().numpy(), ref)
        _same(tris.cpu().numpy(), t)


def test_float32_is_narrowed_once():
    """Loop x3 on a Float32 mesh equals the float64 result narrowed at the end
    and differs from narrowing after every iteration."""
    p, n, c, t = mesh("soup", np.float32)
    once = oracle("soup", "loop", 3, np.float32)
    each = orc.subdivide_loop(p, t, 3, normals=n, colors=c,
                              narrow_each_iteration=True)
    assert not np.array_equal(_bits(once[0]), _bits(each[0]))
    wide = orc.subdivide_loop(p.astype(np.float64), t, 3)
    _same(once[0], wide[0].astype(np.float32))
    check_against_oracle("soup", "loop", 3, np.float32)


# ---- the count / capacity protocol ---------------------------------------------------
@pytest.mark.parametrize("which", ["midpoint", "loop"])
def test_count_then_fill_and_short_capacity(which):
    p, n, c, t = mesh("odd")
    t = t.astype(np.int32)
    want = oracle("odd", which, 2)
    call = getattr(_L().lib(), CALLS[which])
    pd, td = _dev(p), _dev(t)
    n_v, n_t = C.c_int64(-5), C.c_int64(-5)
    st = call(_p(pd), len(p), F64, None, None, F64, _p(td), len(t), I32, 2,
              None, None, None, -1, None, C.byref(n_v), C.byref(n_t), None)
    assert (st, n_v.value, n_t.value) == (OK, len(want[0]), 16 * len(t))
    # the walk's count, not E' = 2 E + 3 M: (3,3,4) and (5,5,5) name self edges
    for capacity in (n_v.value - 1, 0):
        st, outs, tris, got_v, got_t = abi(which, p, n, c, t, 2, capacity)
        assert st == CAPACITY
        assert (got_v, got_t) == (len(want[0]), 16 * len(t))
        assert all(_poisoned(o) for o in outs) and _poisoned(tris)
    check_against_oracle("odd", which, 2, slack=5)


# ---- refusals, outputs intact --------------------------------------------------------
def _refused(which, p, n, c, t, iterations, code, attr_code=None,
             tri_rows=None, capacity=None):
    capacity = len(p) + 3 * len(t) if capacity is None else capacity
    st, outs, tris, _, _ = abi(which, p, n, c, t, iterations, capacity,
                               attr_code, tri_rows)
    assert st == code
    assert all(_poisoned(o) for o in outs) and _poisoned(tris)
    return _L().lib().o3dmi_last_error().decode()


@pytest.mark.parametrize("which", ["midpoint", "loop"])
def test_refusals_leave_the_outputs_alone(which):
    p, n, c, t = mesh("odd")
    t = t.astype(np.int32)
    bad = t.copy()
    bad[1, 2] = len(p)
    assert "outside [0, v)" in _refused(which, p, n, c, bad, 1, INVALID_ARG)
    bad[1, 2] = -1
    _refused(which, p, n, c, bad, 1, INVALID_ARG)
    for row in (0, 6):  # a referenced and the unreferenced vertex
        for k in range(3):
            arrays = [p.copy(), n.copy(), c.copy()]
            arrays[k][row, 1] = np.nan if k != 1 else np.inf
            assert "non-finite" in _refused(which, *arrays, t, 1, INVALID_ARG)
    _refused(which, p, n.astype(np.float32), None, t, 1, UNSUPPORTED,
             attr_code=F32)
    _refused(which, p, None, c.astype(np.float32), t, 1, UNSUPPORTED,
             attr_code=F32)


@pytest.mark.parametrize("which", ["midpoint", "loop"])
def test_limits_are_refused_before_anything_is_allocated(which):
    p, _, _, t = mesh("triangle")
    t = t.astype(np.int32)
    # 4^20 triangles: refused at once, from the sizes alone
    msg = _refused(which, p, None, None, t, 20, INVALID_ARG, tri_rows=4,
                   capacity=8)
    assert "2^29" in msg
    msg = _refused(which, p, None, None, t, 2 ** 31 - 1, INVALID_ARG,
                   tri_rows=4, capacity=8)
    assert "2^29" in msg
    # v + (4^n - 1) m vertices at the most: neither array is read
    call = getattr(_L().lib(), CALLS[which])
    pd, td = _dev(p), _dev(t)
    n_v, n_t = C.c_int64(-5), C.c_int64(-5)
    st = call(_p(pd), 2 ** 31 - 4, F64, None, None, F64, _p(td), 2, I32, 1,
              None, None, None, -1, None, C.byref(n_v), C.byref(n_t), None)
    assert st == INVALID_ARG and (n_v.value, n_t.value) == (-5, -5)
    assert "2^31" in _L().lib().o3dmi_last_error().decode()


def test_loop_is_deterministic():
    p, n, c, t = mesh("soup")
    a = abi("loop", p, n, c, t, 2)
    b = abi("loop", p, n, c, t, 2)
    assert a[0] == b[0] == OK and a[3:] == b[3:]
    for x, y in zip(a[1] + [a[2]], b[1] + [b[2]]):
        _same(x.cpu().numpy(), y.cpu().numpy())


# ---- cross-checks through the project's own calls --------------------------------------
def _as_mesh(name, fdt=np.float64, idt=np.int32, positions=None):
    p, n, c, t = mesh(name, fdt)
    p = p if positions is None else positions
    return {"positions": _dev(p), "normals": _dev(n), "colors": _dev(c),
            "indices": _dev(t.astype(idt))}


def test_midpoint_keeps_the_surface_area_of_a_planar_grid():
    v = MESHES["grid33"][0]
    i, j = np.divmod(np.arange(v), 33)
    flat = np.stack([0.37 * i, 0.21 * j + 0.05 * i, np.zeros(v)], axis=1)
    m = _as_mesh("grid33", positions=flat)
    area = _tm().get_surface_area(m)
    assert area > 0
    for iterations in (1, 2):
        got = _tm().get_surface_area(_tm().subdivide_midpoint(m, iterations))
        assert abs(got - area) <= 1e-12 * area


@pytest.mark.parametrize("which", ["midpoint", "loop"])
def test_tetrahedron_keeps_its_topology(which):
    tm = _tm()
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    m = {"positions": _dev(p), "indices": _dev(np.array(TETRA, np.int32))}
    assert tm.euler_poincare_characteristic(m) == 2
    out = getattr(tm, "subdivide_" + which)(m, 3)
    assert out["positions"].shape == (130, 3)
    assert out["indices"].shape == (256, 3)
    assert tm.euler_poincare_characteristic(out) == 2
    assert tm.is_watertight(out) and tm.is_orientable(out)
    if which == "loop":
        assert 0 < tm.get_volume(out) < tm.get_volume(m)


# ---- the Python mirror -------------------------------------------------------------------
@pytest.mark.parametrize("which", ["midpoint", "loop"])
def test_python_mirror(which):
    tm = _tm()
    call = getattr(tm, "subdivide_" + which)
    want = oracle("fan6", which, 2, np.float32)
    m = _as_mesh("fan6", np.float32, np.int64)
    out = call(m, 2)
    assert sorted(out) == ["colors", "indices", "normals", "positions"]
    for name, ref in zip(("positions", "normals", "colors"), want[:3]):
        _same(out[name].cpu().numpy(), ref)
    _same(out["indices"].cpu().numpy(), want[3])
    assert sorted(m) == ["colors", "indices", "normals", "positions"]

    bare = {"positions": m["positions"], "indices": m["indices"]}
    assert sorted(call(bare)) == ["indices", "positions"]
    bare_want = oracle("fan6", which, 1, np.float32, False)
    _same(call(bare)["positions"].cpu().numpy(), bare_want[0])

    with_tn = tm.compute_triangle_normals(bare)
    out = call(with_tn, 1)
    assert sorted(out) == ["indices", "positions", "triangle_normals"]
    again = tm.compute_triangle_normals(
        {"positions": out["positions"], "indices": out["indices"]})
    _same(out["triangle_normals"].cpu().numpy(),
          again["triangle_normals"].cpu().numpy())
    assert out["triangle_normals"].shape == (24, 3)
