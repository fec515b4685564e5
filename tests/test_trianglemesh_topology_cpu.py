"""The numpy / Python restatement of the mesh topology and intersection
queries (tests/_trianglemesh_topology_oracle.py) against the literal vectors
of upstream's own tests (tests/golden/trianglemesh_topology_vectors.json),
its literal transcription of the legacy loops against the brute-force
definitions the C ABI states, its per-pair function against an exact one in
fractions, and the binding of the new C ABI. No GPU."""
import json
import math
import os
import re

import numpy as np
import pytest

import _trianglemesh_topology_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_CALLS = [
    "o3dmi_trianglemesh_euler_poincare_characteristic",
    "o3dmi_trianglemesh_is_edge_manifold",
    "o3dmi_trianglemesh_get_non_manifold_vertices",
    "o3dmi_trianglemesh_orient_triangles",
    "o3dmi_trianglemesh_get_self_intersecting_triangles",
    "o3dmi_trianglemesh_is_self_intersecting",
    "o3dmi_trianglemesh_is_intersecting",
    "o3dmi_trianglemesh_is_watertight",
    "o3dmi_trianglemesh_get_volume",
]


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden",
                           "trianglemesh_topology_vectors.json")) as f:
        return json.load(f)


def _closed_meshes(gold):
    box = (np.array(gold["box"]["vertices"], np.float64),
           np.array(gold["box"]["triangles"], np.int32))
    return {"box": box, "sphere": orc.make_sphere(), "cone": orc.make_cone(20),
            "torus": orc.make_torus()}


# ---- upstream's literals ------------------------------------------------------------
def test_euler_golden(gold):
    for g in gold["euler"]:
        assert orc.euler_poincare_characteristic(
            len(g["vertices"]), g["triangles"]) == g["expected"]
    for name, (p, t) in _closed_meshes(gold).items():
        assert orc.euler_poincare_characteristic(
            len(p), t.tolist()) == gold[name]["euler"], name


def test_edge_manifold_golden(gold):
    for g in gold["edge_manifold"]:
        assert orc.is_edge_manifold(g["triangles"], True) == g["allow_boundary"]
        assert orc.is_edge_manifold(g["triangles"], False) == g["no_boundary"]
    for name, (p, t) in _closed_meshes(gold).items():
        assert orc.is_edge_manifold(t.tolist(), True), name
        assert orc.is_edge_manifold(t.tolist(), False), name


def test_vertex_manifold_golden(gold):
    for g in gold["vertex_manifold"]:
        n = len(g["vertices"])
        assert bool(orc.get_non_manifold_vertices(n, g["triangles"])) != \
            g["expected"]
        assert orc.get_non_manifold_vertices(n, g["triangles"]) == [0]
        assert orc.wedge_non_manifold_vertices(n, g["triangles"]) == [0]
    for name, (p, t) in _closed_meshes(gold).items():
        assert orc.get_non_manifold_vertices(len(p), t.tolist()) == [], name


def test_self_intersecting_golden(gold):
    for g in gold["self_intersecting"]:
        pairs, _ = orc.get_self_intersecting_triangles(g["vertices"],
                                                       g["triangles"])
        assert bool(pairs) == g["expected"], g["name"]
        assert orc.self_intersections(g["vertices"], g["triangles"])[0] == \
            pairs
    for name, (p, t) in _closed_meshes(gold).items():
        assert orc.self_intersections(p, t)[0] == [], name


def test_volume_golden(gold):
    box, sphere = _closed_meshes(gold)["box"], orc.make_sphere()
    assert orc.is_watertight(*box) and orc.canonical_orientation(box[1])[0]
    assert abs(orc.get_volume(*box) - gold["box"]["volume"]) <= \
        gold["box"]["volume_tolerance"]
    # a 2 x 3 x 1 box: every triple product is a multiple of 6, every term
    # and every partial sum an integer
    assert orc.get_volume(box[0] * [2.0, 3.0, 1.0], box[1]) == 6.0
    assert orc.is_watertight(*sphere)
    assert orc.canonical_orientation(sphere[1])[0]
    assert abs(orc.get_volume(*sphere) - 4.0 / 3.0 * math.pi) <= \
        gold["sphere"]["volume_tolerance"]


# ---- the transcription against the definitions -----------------------------------------
def _soup(rng, n_vertices, m, repeated):
    t = rng.integers(0, n_vertices, (m, 3))
    if not repeated:
        t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) &
              (t[:, 2] != t[:, 0])]
    return t.tolist()


def test_non_manifold_vertices_agree_on_soups():
    rng = np.random.default_rng(7)
    seen = 0
    for trial in range(300):
        v = int(rng.integers(3, 9))
        t = _soup(rng, v, int(rng.integers(1, 14)), True)
        want = orc.wedge_non_manifold_vertices(v, t)
        assert orc.get_non_manifold_vertices(v, t) == want, t
        seen += bool(want)
    assert seen >= 30


def _multiplicity_at_most_two(t):
    return all(len(x) <= 2 for x in orc.edge_to_triangles(t).values())


def test_orientation_agrees_on_soups():
    """Both decide orientability alike where upstream is a function of the
    mesh (every edge in at most two triangles, no repeated vertex), and the
    flip sets are the same up to each row's rotation."""
    rng = np.random.default_rng(11)
    compared = orientable = 0
    for trial in range(6000):
        v = int(rng.integers(5, 8))
        t = _soup(rng, v, int(rng.integers(5, 11)), False)
        if len(t) < 2 or not _multiplicity_at_most_two(t):
            continue
        ok_up, tris_up = orc.orient_triangles(t)
        ok, tris = orc.canonical_orientation(t)
        assert ok_up == ok, t
        compared += 1
        if ok:
            orientable += 1
            assert [orc.rotate_min_first(x) for x in tris_up] == \
                [orc.rotate_min_first(x) for x in tris], t
    assert compared >= 200 and orientable >= 50
    assert compared - orientable >= 5


def test_orientation_of_closed_meshes_with_flips(gold):
    rng = np.random.default_rng(3)
    for name, (p, t) in _closed_meshes(gold).items():
        flipped = t.copy()
        pick = rng.random(len(t)) < 0.4
        pick[0] = False
        flipped[pick] = flipped[pick][:, [0, 2, 1]]
        ok, tris = orc.canonical_orientation(flipped)
        assert ok, name
        assert np.array_equal(np.array(tris), t), name
        assert orc.orient_triangles(flipped)[0], name


def test_mobius_and_fan_are_not_orientable():
    for n in (5, 8, 13):
        _, t = orc.make_mobius(n)
        assert _multiplicity_at_most_two(t.tolist())
        assert not orc.canonical_orientation(t)[0]
        assert not orc.orient_triangles(t)[0]
    fan = [[0, 1, 2], [0, 1, 3], [0, 1, 4]]
    ok, tris = orc.canonical_orientation(fan)
    assert not ok and tris == fan


# ---- the per-pair function against an exact one ------------------------------------------
def test_per_pair_function_against_fractions():
    rng = np.random.default_rng(5)
    hits = misses = 0
    for trial in range(4000):
        p = rng.random((3, 3))
        q = rng.random((3, 3)) * 0.8 + rng.random(3) * 0.4
        if orc.min_plane_distance(p, q) <= 1e-3:
            continue
        want = orc.exact_intersects(p, q)
        assert orc.triangle_triangle_3d(p.tolist(), q.tolist()) == want
        # intersecting triangles have overlapping boxes
        assert orc.pair_counts(p.tolist(), q.tolist()) == want
        hits += want
        misses += not want
        if hits >= 200 and misses >= 200:
            break
    assert hits >= 200 and misses >= 200, (hits, misses)


def test_box_candidates_match_the_loop():
    rng = np.random.default_rng(9)
    c = rng.random((60, 1, 3))
    p = (c + (rng.random((60, 3, 3)) - 0.5) * 0.3).reshape(-1, 3)
    t = np.arange(180).reshape(60, 3)
    pairs, tested = orc.get_self_intersecting_triangles(p, t)
    assert (pairs, tested) == orc.self_intersections(p, t)
    assert 0 < len(pairs) < tested


# ---- the C ABI ------------------------------------------------------------------------------
def test_new_calls_are_declared_and_bound():
    from open3d_amd import _lib
    txt = open(os.path.join(ROOT, "include", "o3d_mi355x_host.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(o3dmi_[a-z0-9_]+)\s*\(", txt))
    for name in NEW_CALLS:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
    assert "o3dmi_internal_trianglemesh_self_intersections" in \
        _lib.INTERNAL_PROTOTYPES
