"""CPU tests of the rules behind TriangleMesh sampling, closest points and
ComputeMetrics: the exported draw against the numpy restatement
(tests/_mesh_distance_oracle.py), the restatement's prefix-tree descent and
per-pair function against hand-made cases and an independent float64
evaluation, upstream's literal vectors (tests/golden/
mesh_distance_vectors.json), and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import _mesh_distance_oracle as orc

F32 = np.float32
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 7
F32_CODE, F64_CODE, I32_CODE = 0, 1, 4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from open3d_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def gold():
    return orc.golden()


# ---- the draw ------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2024, 0x9E3779B97F4A7C15, 2 ** 64 - 1])
@pytest.mark.parametrize("j", [0, 1, 2, 2 ** 32, 2 ** 62])
def test_draw_is_the_restatement(L, seed, j):
    u, r1, r2 = C.c_double(-1), C.c_float(-1), C.c_float(-1)
    assert L.o3dmi_mesh_sample_draw(seed, j, C.byref(u), C.byref(r1),
                                    C.byref(r2)) == OK
    wu, w1, w2 = orc.draw(seed, j)
    assert np.float64(u.value).tobytes() == np.float64(wu).tobytes()
    assert F32(r1.value).tobytes() == F32(w1).tobytes()
    assert F32(r2.value).tobytes() == F32(w2).tobytes()
    assert 0.0 <= u.value < 1.0
    assert 0.0 <= r1.value < 1.0 and 0.0 <= r2.value < 1.0


def test_draw_ranges_and_errors(L):
    us, r1s = [], []
    for j in range(2000):
        u, r1, r2 = orc.draw(7, j)
        assert 0.0 <= u < 1.0 and F32(0) <= r1 < F32(1) and F32(0) <= r2 < F32(1)
        us.append(u)
        r1s.append(r1)
    # 2000 uniform draws: the mean lies within 5 sigma = 5 / sqrt(12 * 2000)
    assert abs(np.mean(us) - 0.5) < 5 / np.sqrt(12 * 2000)
    assert abs(np.mean(r1s) - 0.5) < 5 / np.sqrt(12 * 2000)
    # the largest values the rule can give are below 1
    assert np.float64(2 ** 53 - 1) * np.float64(2.0 ** -53) < 1.0
    assert F32(2 ** 24 - 1) * F32(2.0 ** -24) < F32(1)
    u, r1, r2 = C.c_double(-1), C.c_float(-1), C.c_float(-1)
    assert L.o3dmi_mesh_sample_draw(0, -1, C.byref(u), C.byref(r1),
                                    C.byref(r2)) == INVALID_ARG
    assert L.o3dmi_mesh_sample_draw(0, 0, None, C.byref(r1),
                                    C.byref(r2)) == INVALID_ARG
    assert (u.value, r1.value, r2.value) == (-1, -1, -1)


# ---- the descent ---------------------------------------------------------------
U_LAST = np.nextafter(np.float64(1), np.float64(0))  # the largest double < 1
US = [0.0, 0.25, 0.5, 0.75, U_LAST]


def _picks(areas, us=US):
    levels = orc.prefix_levels(np.asarray(areas, np.float64))
    return [orc.descend(levels, u) for u in us]


def test_descent_one_triangle():
    assert _picks([3.0]) == [0] * len(US)


@pytest.mark.parametrize("m", [512, 513])
def test_descent_at_the_group_edge(m):
    areas = np.ones(m)
    levels = orc.prefix_levels(areas)
    assert len(levels) == (1 if m <= 512 else 2)
    assert orc.total_area(levels) == m
    for u in US + [511.5 / m, 512.0 / m, 512.5 / m]:
        u = min(u, U_LAST)
        # unit areas: the prefixes are exact, triangle floor(x) of x = u m
        x = np.float64(u) * np.float64(m)
        assert x < m
        assert orc.descend(levels, u) == int(np.floor(x))


def test_descent_skips_a_whole_zero_group():
    areas = np.concatenate([np.ones(512), np.zeros(512), np.ones(512)])
    levels = orc.prefix_levels(areas)
    assert len(levels) == 2 and orc.total_area(levels) == 1024
    assert orc.descend(levels, 0.0) == 0
    assert orc.descend(levels, 0.5 - 2.0 ** -12) == 511
    assert orc.descend(levels, 0.5) == 1024  # the first of the third group
    assert orc.descend(levels, U_LAST) == 1535
    rng = np.random.default_rng(5)
    for u in rng.random(500):
        t = orc.descend(levels, u)
        assert not 512 <= t < 1024


def test_descent_never_returns_a_zero_area_triangle():
    rng = np.random.default_rng(11)
    areas = rng.random(1500)
    areas[rng.random(1500) < 0.5] = 0.0
    areas[0] = areas[-1] = 0.0  # u = 0 and u -> 1 land next to zeros
    areas[510:515] = 0.0
    levels = orc.prefix_levels(areas)
    for u in list(rng.random(2000)) + [0.0, U_LAST]:
        assert areas[orc.descend(levels, u)] > 0


def test_descent_rounding_fallback():
    # When no prefix of a group is above x the rule takes the last member
    # with a value > 0. u = 1 is outside the draw's range; it stands in for
    # an x that rounding left at the group's total.
    areas = np.array([0.1, 0.7, 0.0, 0.0])
    levels = orc.prefix_levels(areas)
    assert orc.descend(levels, U_LAST) == 1
    assert orc.descend(levels, 1.0) == 1
    areas = np.concatenate([np.ones(512), [1.0, 2.0, 0.0]])
    levels = orc.prefix_levels(areas)
    assert orc.descend(levels, 1.0) == 513


def test_descent_follows_the_areas(gold):
    """The distribution check the GPU test repeats with the same seed: two
    triangles of area 1 : 3, n = 100000 draws, the count on the first within
    5 sigma of n / 4 (sigma = sqrt(n 1/4 3/4) ~ 137: within 685)."""
    g = gold["area_ratio"]
    pos, tri = np.array(g["positions"], F32), np.array(g["triangles"])
    n, seed = g["n"], g["seed"]
    areas = orc.tm.triangle_areas(pos, tri)
    assert list(areas) == [1.0, 3.0]
    levels = orc.prefix_levels(areas)
    first = sum(orc.descend(levels, orc.draw(seed, j)[0]) == 0
                for j in range(n))
    sigma = np.sqrt(n * 0.25 * 0.75)
    assert abs(first - n / 4) <= 5 * sigma, first


# ---- the per-pair function -----------------------------------------------------
def _lattice_distance(q, a, b, c, steps):
    """min |q - (a + u ab + v ac)| over the lattice u, v = i / steps, u + v <=
    1, in float64."""
    q, a, b, c = (np.asarray(x, np.float64) for x in (q, a, b, c))
    i = np.arange(steps + 1)
    u, v = np.meshgrid(i, i, indexing="ij")
    keep = u + v <= steps
    u, v = u[keep] / steps, v[keep] / steps
    p = a + u[:, None] * (b - a) + v[:, None] * (c - a)
    return np.sqrt(((p - q) ** 2).sum(axis=1).min())


def _check_against_lattice(q, a, b, c, tol32):
    steps = 512
    d2, point, u, v, e2, b2 = orc.pair_d2(q, a, b, c)
    d = np.sqrt(np.float64(d2))
    lat = _lattice_distance(q, a, b, c, steps)
    edge = max(np.linalg.norm(np.float64(b) - np.float64(a)),
               np.linalg.norm(np.float64(c) - np.float64(a)))
    # Every point of the triangle is within h (|ab| + |ac|) <= 2 L h of a
    # lattice point (h = 1 / steps, L the longer of the two edges), so the
    # true distance d* satisfies lat - 2 L h <= d* <= lat; tol32 bounds the
    # float32 evaluation's own error.
    assert lat - 2 * edge / steps - tol32 <= d <= lat + tol32, (d, lat)
    # the reported point is the one the distance belongs to, unless the box
    # clamp took over
    if e2 >= b2:
        assert abs(np.linalg.norm(np.float64(q) - np.float64(point)) - d) \
            <= tol32


def test_pair_function_on_random_triangles():
    rng = np.random.default_rng(3)
    eps = float(np.finfo(F32).eps)
    done = 0
    while done < 150:
        a, b, c, q = (rng.uniform(-1, 1, 3).astype(F32) for _ in range(4))
        ab, ac, bc = (np.linalg.norm(x) for x in (b - a, c - a, c - b))
        area = 0.5 * np.linalg.norm(np.cross(b - a, c - a))
        if min(ab, ac, bc) < 0.3 or area < 0.1:
            continue
        # Coordinates and differences are below S = 4 in magnitude; every
        # dot product, and va, vb, vc (products of two of them, S^4), carry a
        # few eps relative to that, and the barycentric coordinates divide by
        # (2 area)^2 >= 0.04 or an edge^2 >= 0.09: 256 eps S covers it.
        _check_against_lattice(q, a, b, c, 256 * eps * 4.0)
        done += 1


def test_pair_function_on_sliver_triangles():
    rng = np.random.default_rng(4)
    eps = float(np.finfo(F32).eps)
    aspect = 1e-3
    for _ in range(100):
        a = rng.uniform(-1, 1, 3).astype(F32)
        dirn = rng.standard_normal(3)
        dirn /= np.linalg.norm(dirn)
        side = np.cross(dirn, rng.standard_normal(3))
        side /= np.linalg.norm(side)
        b = (a + dirn).astype(F32)
        c = (a + rng.uniform(0.2, 0.8) * dirn + aspect * side).astype(F32)
        q = rng.uniform(-1.5, 1.5, 3).astype(F32)
        # As above with the height of the triangle, aspect, in place of a
        # length of order 1 in the interior branch's denominator: the
        # barycentric error grows by 1 / aspect, and so does the bound. The
        # box clamp keeps d2 from falling below the box distance whatever
        # the cancellation does.
        _check_against_lattice(q, a, b, c, 256 * eps * 4.0 / aspect)
        d2, _, _, _, e2, b2 = orc.pair_d2(q, a, b, c)
        assert d2 >= b2


def test_seven_voronoi_branches():
    a, b, c = [0, 0, 0], [1, 0, 0], [0, 1, 0]
    cases = [  # query, branch, closest point, (u, v)
        ([-1, -1, 0], 0, [0, 0, 0], (0, 0)),
        ([2, -0.5, 0], 1, [1, 0, 0], (1, 0)),
        ([-0.5, 2, 0], 2, [0, 1, 0], (0, 1)),
        ([0.5, -1, 0], 3, [0.5, 0, 0], (0.5, 0)),
        ([-1, 0.5, 0], 4, [0, 0.5, 0], (0, 0.5)),
        ([1, 1, 0], 5, [0.5, 0.5, 0], (0.5, 0.5)),
        ([0.25, 0.25, 1], 6, [0.25, 0.25, 0], (0.25, 0.25)),
    ]
    seen = set()
    for q, branch, point, uv in cases:
        p, u, v, br = orc.closest_point_triangle(q, a, b, c)
        assert int(br) == branch
        assert np.array_equal(p, np.array(point, F32))
        assert (float(u), float(v)) == uv
        d2 = orc.pair_d2(q, a, b, c)[0]
        want = np.float64(np.sum((np.array(q) - np.array(point)) ** 2))
        assert float(d2) == want  # dyadic values: exact in float32
        seen.add(branch)
    assert seen == set(range(7))


def test_degenerate_triangles_follow_upstreams_statements():
    # a == b: ab = 0, so d1 = d3 = 0 and d4 = d2. Behind a (d2 <= 0) the
    # first branch returns a. Past c (d6 >= 0, d5 = 0 <= d6) the third returns
    # c. Between them vc = d1 d4 - d3 d2 = 0 passes the edge test of ab and
    # v = d1 / (d1 - d3) = 0 / 0: NaN, which upstream's `d < radius` rejects.
    a = b = [0, 0, 0]
    c = [2, 0, 0]
    d2, p, _, _, _, _ = orc.pair_d2([-1, 1, 0], a, b, c)
    assert float(d2) == 2.0 and np.array_equal(p, np.zeros(3, F32))
    d2, p, _, _, _, _ = orc.pair_d2([3, 1, 0], a, b, c)
    assert float(d2) == 2.0 and np.array_equal(p, np.array(c, F32))
    d2, p, _, _, _, _ = orc.pair_d2([1, 1, 0], a, b, c)
    assert np.isnan(d2) and np.isnan(p).all()
    # collinear a, b, c = 0, 1, 2 on the x axis, query above 0.5: d1 = 0.5,
    # d2 = 1, d3 = -0.5, d4 = -1, vc = -0.5 + 0.5 = 0 -> the ab branch,
    # v = 0.5 / 1: finite
    d2, p, u, v, _, _ = orc.pair_d2([0.5, 1, 0], [0, 0, 0], [1, 0, 0],
                                    [2, 0, 0])
    assert float(d2) == 1.0 and np.array_equal(p, np.array([0.5, 0, 0], F32))
    assert (float(u), float(v)) == (0.5, 0.0)
    # every vertex at one point: the first or the second branch, never NaN
    for q in ([1, 2, 3], [0, 0, 0], [-1, 0, 0]):
        d2 = orc.pair_d2(q, [0, 0, 0], [0, 0, 0], [0, 0, 0])[0]
        assert float(d2) == float(np.sum(np.array(q, np.float64) ** 2))
    # a NaN pair never wins the exhaustive loop, and a mesh of nothing else
    # gives the "no triangle" row
    pos = np.array([[0, 0, 0], [0, 0, 0], [2, 0, 0], [5, 5, 5], [6, 5, 5],
                    [5, 6, 5]], F32)
    got = orc.closest_points(pos, [[0, 1, 2], [3, 4, 5]], [[1, 1, 0]])
    assert got["primitive_ids"][0] == 1
    got = orc.closest_points(pos, [[0, 1, 2]], [[1, 1, 0]])
    assert got["primitive_ids"][0] == orc.NO_TRIANGLE
    assert got["distance"][0] == np.inf and not got["points"].any()


def test_ties_go_to_the_lowest_index(gold):
    pos, tri = orc.unit_cube()
    got = orc.closest_points(pos, tri, [[0.5, 0.5, 0.5], [0.5, 0, 0]])
    assert list(got["primitive_ids"]) == [0, 4]
    assert list(got["distance"]) == [0.5, 0.0]


# ---- upstream's vectors --------------------------------------------------------
def test_upstream_closest_point_vectors(gold):
    g = gold["closest_points"]
    got = orc.closest_points(np.array(g["positions"], F32), g["triangles"],
                             np.array(g["queries"], F32))
    np.testing.assert_allclose(got["points"], np.array(g["points"]),
                               rtol=g["rtol"], atol=g["atol"])
    assert list(got["primitive_ids"]) == g["primitive_ids"]


def test_upstream_cube_distances(gold):
    g = gold["cube"]
    pos, tri = orc.unit_cube()
    # the hand-written cube is closed and outward: every edge twice, area 6
    assert orc.tm.non_manifold_edges(tri, allow_boundary_edges=False).size == 0
    assert orc.tm.surface_area(pos, tri) == 6.0
    got = orc.closest_points(pos, tri, np.array(g["queries"], F32))
    np.testing.assert_allclose(got["distance"], np.array(g["distance"]),
                               rtol=g["rtol"])


# ---- argument checks that reach no device ----------------------------------------
def test_argument_errors_before_any_device_work(L):
    one = C.c_void_p(256)  # never dereferenced: the checks come first
    handle = C.c_void_p()
    create = L.o3dmi_mesh_bvh_create
    assert create(one, 3, F64_CODE, one, 1, I32_CODE, C.byref(handle),
                  None) == UNSUPPORTED
    assert create(one, 3, F32_CODE, one, 0, I32_CODE, C.byref(handle),
                  None) == INVALID_ARG
    assert create(one, 3, F32_CODE, one, -1, I32_CODE, C.byref(handle),
                  None) == INVALID_ARG
    assert create(None, 3, F32_CODE, one, 1, I32_CODE, C.byref(handle),
                  None) == INVALID_ARG
    assert create(one, 3, F32_CODE, one, 1, F32_CODE, C.byref(handle),
                  None) == INVALID_ARG
    assert create(one, 3, F32_CODE, one, 1, I32_CODE, None,
                  None) == INVALID_ARG
    assert handle.value is None
    assert L.o3dmi_mesh_bvh_destroy(None) == OK
    assert L.o3dmi_mesh_bvh_closest_points(None, one, 1, F32_CODE, one, None,
                                           None, None, None,
                                           None) == INVALID_ARG
    sample = L.o3dmi_trianglemesh_sample_points_uniformly
    tail = (0, None, None, None, 0, one, None, None, None, None)
    assert sample(one, 3, F32_CODE, one, 1, I32_CODE, 0, *tail) == INVALID_ARG
    assert sample(one, 3, F32_CODE, one, 0, I32_CODE, 5, *tail) == INVALID_ARG
    assert sample(one, 0, F32_CODE, one, 1, I32_CODE, 5, *tail) == INVALID_ARG
    assert sample(one, 3, F32_CODE, one, 1, I32_CODE, 5, 0, None, None, None,
                  0, None, None, None, None, None) == INVALID_ARG
    # normals wanted, none given
    assert sample(one, 3, F32_CODE, one, 1, I32_CODE, 5, 0, None, None, None,
                  0, one, one, None, None, None) == INVALID_ARG
    metrics = (C.c_int * 1)(0)
    values = (C.c_float * 1)(-7)
    cm = L.o3dmi_trianglemesh_compute_metrics
    assert cm(one, 3, one, 1, I32_CODE, one, 3, one, 1, I32_CODE, F64_CODE,
              metrics, 1, None, 0, 10, 0, values, 1, None, None) == UNSUPPORTED
    assert cm(one, 3, one, 1, I32_CODE, one, 3, one, 0, I32_CODE, F32_CODE,
              metrics, 1, None, 0, 10, 0, values, 1, None, None) == INVALID_ARG
    assert cm(one, 3, one, 1, I32_CODE, one, 3, one, 1, I32_CODE, F32_CODE,
              metrics, 1, None, 0, 0, 0, values, 1, None, None) == INVALID_ARG
    assert values[0] == -7
