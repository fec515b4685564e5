"""CPU tests of the rules behind the ray queries on a mesh: the numpy
restatement (tests/_mesh_ray_oracle.py) against upstream's literal vectors
(tests/golden/raycasting_vectors.json) and against itself (count, list and
unique(t) agree), the exported vote directions against the restatement bit
for bit, and the declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _mesh_ray_oracle as orc

F32 = np.float32
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 7
F32_CODE, F64_CODE = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ["o3dmi_mesh_bvh_cast_rays", "o3dmi_mesh_bvh_test_occlusions",
          "o3dmi_mesh_bvh_count_intersections",
          "o3dmi_mesh_bvh_list_intersections",
          "o3dmi_mesh_bvh_compute_occupancy",
          "o3dmi_mesh_bvh_compute_signed_distance",
          "o3dmi_raycast_vote_directions", "o3dmi_create_rays_pinhole",
          "o3dmi_trianglemesh_cast_rays",
          "o3dmi_trianglemesh_compute_signed_distance"]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from open3d_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def gold():
    return orc.golden()


def _num(x):
    return np.inf if x == "inf" else x


# ---- upstream's vectors through the restatement ----------------------------------
def test_upstream_triangle_vectors(gold):
    g = gold["triangle"]
    pos, tri, rays = g["positions"], g["triangles"], np.array(g["rays"], F32)
    got = orc.cast_rays(pos, tri, rays)
    want = g["cast_rays"]
    assert got["geometry_ids"].tolist() == want["geometry_ids"]
    assert got["primitive_ids"].tolist() == [0, gold["invalid_id"]]
    assert np.isclose(got["t_hit"][0], want["t_hit"][0],
                      rtol=want["t_hit_rtol"], atol=want["t_hit_atol"])
    assert got["t_hit"][1] == np.inf
    assert not got["primitive_uvs"][1].any()
    assert not got["primitive_normals"][1].any()
    # u weighs vertex 1 and v vertex 2: the hit point from the coordinates
    u, v = got["primitive_uvs"][0].astype(np.float64)
    p = np.array(pos, np.float64)
    hit = (1 - u - v) * p[0] + u * p[1] + v * p[2]
    np.testing.assert_allclose(hit, [0.2, 0.1, 0.0], atol=1e-6)
    assert got["primitive_normals"][0].tolist() == [0.0, 0.0, 1.0]
    for case in g["occlusions"]:
        got = orc.occlusions(pos, tri, rays, _num(case["tnear"]),
                             _num(case["tfar"]))
        assert got.tolist() == case["occluded"], case


def test_upstream_box_vectors(gold):
    g = gold["box"]
    pos, tri = orc.unit_box()
    rays = np.array(g["rays"], F32)
    assert orc.count_intersections(pos, tri, rays).tolist() == g["counts"]
    lst = orc.list_intersections(pos, tri, rays)
    np.testing.assert_allclose(lst["t_hit"], g["list_t_hit"],
                               rtol=g["list_tolerance"],
                               atol=g["list_tolerance"])
    assert lst["ray_splits"].tolist() == [0, 2, 3, 3]
    assert lst["ray_ids"].tolist() == [0, 0, 1]
    for nsamples in (1, 3):
        sd = orc.compute_signed_distance(
            pos, tri, np.array(g["signed_distance_queries"], F32), nsamples)
        np.testing.assert_allclose(sd, g["signed_distance"],
                                   rtol=g["signed_distance_rtol"])
        occ = orc.compute_occupancy(
            pos, tri, np.array(g["occupancy_queries"], F32), nsamples)
        assert occ.tolist() == g["occupancy"]


def test_upstream_output_shapes(gold):
    g = gold["output_shapes"]
    pos, tri = gold["triangle"]["positions"], gold["triangle"]["triangles"]
    rs = np.random.RandomState(g["random_state"])
    for shape in g["shapes"]:
        rays = rs.uniform(size=shape + [6]).astype(F32)
        n = int(np.prod(shape))
        assert orc.count_intersections(pos, tri, rays).shape == (n,)
        cast = orc.cast_rays(pos, tri, rays)
        for k, v in cast.items():
            assert list(v.shape) == [n] + g["last_dim"][k], k
        lst = orc.list_intersections(pos, tri, rays)
        total = int(orc.count_intersections(pos, tri, rays).sum())
        for k, v in lst.items():
            first = n + 1 if k == "ray_splits" else total
            assert list(v.shape) == [first] + g["last_dim"][k], k


# ---- the restatement against itself ------------------------------------------------
def test_count_list_and_unique_agree_on_a_soup():
    pos, tri = orc.soup(120, seed=3)
    rays = orc.aimed_rays(80, seed=4)
    counts = orc.count_intersections(pos, tri, rays)
    lst = orc.list_intersections(pos, tri, rays)
    hit, t, _, _ = orc.pairs(pos, tri, rays)
    assert counts.sum() > 40  # the soup is dense enough to be a test
    for r in range(len(rays)):
        lo, hi = lst["ray_splits"][r], lst["ray_splits"][r + 1]
        unique = np.unique(t[r, hit[r]])
        assert counts[r] == hi - lo == len(unique)
        assert lst["t_hit"][lo:hi].tolist() == unique.tolist()
        assert (lst["ray_ids"][lo:hi] == r).all()
    # the closest hit is the first entry of the list
    cast = orc.cast_rays(pos, tri, rays)
    some = counts > 0
    first = lst["ray_splits"][:-1][some]
    assert cast["t_hit"][some].tolist() == lst["t_hit"][first].tolist()
    assert cast["primitive_ids"][some].tolist() == \
        lst["primitive_ids"][first].tolist()
    assert (cast["t_hit"][~some] == np.inf).all()
    # degenerate triangles never hit
    assert not hit[:, 1::4].any()


def test_pair_rules_by_hand():
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
    tri = [[0, 1, 2]]

    def hits(ray, tnear=0.0, tfar=np.inf):
        return bool(orc.pairs(pos, tri, [ray], tnear, tfar)[0][0, 0])
    ray = [0.25, 0.25, 2, 0, 0, -1]
    assert hits(ray) and orc.pairs(pos, tri, [ray])[1][0, 0] == 2.0
    assert hits(ray, tfar=2.0) and not hits(ray, tfar=1.999)  # closed above
    assert not hits(ray, tnear=2.0) and hits(ray, tnear=1.999)  # open below
    assert not hits([0.25, 0.25, 0, 0, 0, -1])  # starts on the surface
    assert hits([0.25, 0.25, -2, 0, 0, 1])  # no back-face culling
    assert not hits([0.25, 0.25, 2, 0, 0, 0])  # zero direction
    assert not hits([0.25, 0.25, 2, 1, 0, 0])  # parallel
    assert hits([0, 0, 2, 0, 0, -1])  # through a vertex
    # t is in units of |d|
    assert orc.pairs(pos, tri, [[0.25, 0.25, 2, 0, 0, -4]])[1][0, 0] == 0.5
    # a duplicated triangle does not raise the count, the lowest index wins
    two = [[0, 1, 2], [0, 1, 2]]
    assert orc.count_intersections(pos, two, [ray]).tolist() == [1]
    assert orc.cast_rays(pos, two, [ray])["primitive_ids"].tolist() == [0]


# ---- the vote directions ---------------------------------------------------------------
def test_mt19937_words_are_the_engines():
    # std::mt19937's 10000th word with the default seed is 4123659995
    # ([rand.predef]); RandomState(5489) must walk the same sequence
    words = orc.mt19937_words(5489, 10000)
    assert int(words[-1]) == 4123659995


@pytest.mark.parametrize("nsamples", [1, 3, 5])
def test_vote_directions_are_the_restatement(L, nsamples):
    out = (C.c_float * (3 * nsamples))(*([-7.0] * (3 * nsamples)))
    assert L.o3dmi_raycast_vote_directions(nsamples, out) == OK
    got = np.array(list(out), F32).reshape(nsamples, 3)
    want = orc.vote_directions(nsamples)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert (np.abs(got - 1) <= F32(0.0011)).all() and (got != 1).any()
    # the first directions do not depend on how many are drawn
    assert got[0].tobytes() == orc.vote_directions(1)[0].tobytes()


def test_vote_directions_refuse_even_and_non_positive(L):
    out = (C.c_float * 12)(*([-7.0] * 12))
    for bad in (0, 2, 4, -1, -3):
        assert L.o3dmi_raycast_vote_directions(bad, out) == INVALID_ARG
    assert L.o3dmi_raycast_vote_directions(1, None) == INVALID_ARG
    assert list(out) == [-7.0] * 12


# ---- the pinhole restatement ------------------------------------------------------------
def test_pinhole_restatement_by_hand():
    k = [[2.0, 0, 1.0], [0, 2.0, 1.0], [0, 0, 1]]
    rays = orc.create_rays_pinhole(k, np.eye(4), 2, 2)
    assert rays.shape == (2, 2, 6) and rays.dtype == F32
    assert not rays[..., :3].any()
    # K^-1 (x + 0.5, y + 0.5, 1) = ((x + 0.5 - 1) / 2, (y + 0.5 - 1) / 2, 1)
    assert rays[0, 0, 3:].tolist() == [-0.25, -0.25, 1.0]
    assert rays[1, 0, 3:].tolist() == [-0.25, 0.25, 1.0]
    assert rays[0, 1, 3:].tolist() == [0.25, -0.25, 1.0]
    # a camera moved by t sees from C = -R^T t
    e = np.eye(4)
    e[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    e[:3, 3] = [1, 2, 3]
    rays = orc.create_rays_pinhole(k, e, 1, 1)
    np.testing.assert_array_equal(rays[0, 0, :3],
                                  (-e[:3, :3].T @ e[:3, 3]).astype(F32))
    inv = orc.inverse3([[500, 0.5, 320], [0, 510, 240], [0, 0, 1]])
    np.testing.assert_allclose(
        inv, np.linalg.inv([[500, 0.5, 320], [0, 510, 240], [0, 0, 1]]),
        rtol=1e-14, atol=1e-17)


# ---- declarations and argument checks that reach no device -----------------------------
def test_symbols_are_declared_and_bound(L):
    from open3d_amd import _lib
    with open(os.path.join(ROOT, "include", "o3d_mi355x_host.h")) as f:
        header = f.read()
    for name in PUBLIC:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert getattr(L, name) is not None
    assert "O3DMI_RAYCAST_INVALID_ID 0xFFFFFFFFu" in header
    with open(os.path.join(ROOT, "open3d_amd", "csrc", "mesh_bvh.h")) as f:
        seam = f.read()
    name = "o3dmi_internal_mesh_bvh_ray_query"
    assert name in seam and name in _lib.INTERNAL_PROTOTYPES
    from open3d_amd import trianglemesh as tm
    assert tm.INVALID_ID == 0xFFFFFFFF
    for method in ("cast_rays", "test_occlusions", "count_intersections",
                   "list_intersections", "compute_occupancy",
                   "compute_signed_distance"):
        assert callable(getattr(tm.MeshBVH, method)), method
    assert callable(tm.create_rays_pinhole)


def test_argument_errors_before_any_device_work(L):
    one = C.c_void_p(256)  # never dereferenced: the checks come first
    total = C.c_int64(-7)
    assert L.o3dmi_mesh_bvh_cast_rays(None, one, 1, F32_CODE, one, None, None,
                                      None, None, None) == INVALID_ARG
    assert L.o3dmi_mesh_bvh_cast_rays(one, one, 1, F64_CODE, one, None, None,
                                      None, None, None) == UNSUPPORTED
    assert L.o3dmi_mesh_bvh_cast_rays(one, one, -1, F32_CODE, one, None, None,
                                      None, None, None) == INVALID_ARG
    assert L.o3dmi_mesh_bvh_cast_rays(one, None, 1, F32_CODE, one, None, None,
                                      None, None, None) == INVALID_ARG
    assert L.o3dmi_mesh_bvh_cast_rays(one, one, 0, F32_CODE, None, None, None,
                                      None, None, None) == OK
    occ = L.o3dmi_mesh_bvh_test_occlusions
    nan, inf = float("nan"), float("inf")
    assert occ(one, one, 1, F32_CODE, nan, inf, one, None) == INVALID_ARG
    assert occ(one, one, 1, F32_CODE, 0.0, nan, one, None) == INVALID_ARG
    assert occ(one, one, 1, F64_CODE, 0.0, inf, one, None) == UNSUPPORTED
    assert occ(one, one, 1, F32_CODE, 0.0, inf, None, None) == INVALID_ARG
    assert occ(one, one, 0, F32_CODE, 0.0, inf, None, None) == OK
    cnt = L.o3dmi_mesh_bvh_count_intersections
    assert cnt(one, one, 1, F64_CODE, one, None) == UNSUPPORTED
    assert cnt(one, one, 1, F32_CODE, None, None) == INVALID_ARG
    lst = L.o3dmi_mesh_bvh_list_intersections
    assert lst(one, one, 1, F32_CODE, None, -1, None, None, None, None, None,
               None, None) == INVALID_ARG
    assert lst(one, one, 1, F64_CODE, None, -1, C.byref(total), None, None,
               None, None, None, None) == UNSUPPORTED
    assert total.value == -7
    assert lst(one, one, 0, F32_CODE, None, -1, C.byref(total), None, None,
               None, None, None, None) == OK
    assert total.value == 0
    for fn in (L.o3dmi_mesh_bvh_compute_occupancy,
               L.o3dmi_mesh_bvh_compute_signed_distance):
        for bad in (0, 2, -1):
            assert fn(one, one, 1, F32_CODE, bad, one, None) == INVALID_ARG
            assert fn(one, one, 0, F32_CODE, bad, one, None) == INVALID_ARG
        assert fn(one, one, 1, F64_CODE, 1, one, None) == UNSUPPORTED
        assert fn(one, one, 1, F32_CODE, 1, None, None) == INVALID_ARG
        assert fn(one, one, 0, F32_CODE, 3, None, None) == OK
    k = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    singular = (C.c_double * 9)(1, 0, 0, 0, 0, 0, 0, 0, 1)
    e = (C.c_double * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1)
    bad_e = (C.c_double * 16)(nan, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0,
                              1)
    pin = L.o3dmi_create_rays_pinhole
    assert pin(None, e, 1, 1, one, None) == INVALID_ARG
    assert pin(k, e, 0, 1, one, None) == INVALID_ARG
    assert pin(k, e, 1, -1, one, None) == INVALID_ARG
    assert pin(k, e, 1, 1, None, None) == INVALID_ARG
    assert pin(singular, e, 1, 1, one, None) == INVALID_ARG
    assert pin(k, bad_e, 1, 1, one, None) == INVALID_ARG
    sd = L.o3dmi_trianglemesh_compute_signed_distance
    assert sd(one, 3, F32_CODE, one, 1, 4, one, 1, 2, one,
              None) == INVALID_ARG
    assert sd(one, 3, F64_CODE, one, 1, 4, one, 1, 1, one,
              None) == UNSUPPORTED
    cast = L.o3dmi_trianglemesh_cast_rays
    assert cast(one, 3, F32_CODE, one, 0, 4, one, 1, one, None, None, None,
                None, None) == INVALID_ARG
    assert cast(one, 3, F64_CODE, one, 1, 4, one, 1, one, None, None, None,
                None, None) == UNSUPPORTED
