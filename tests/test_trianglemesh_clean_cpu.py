"""The numpy restatement of the mesh clean-up calls, the adjacency list, the
smoothing filters and the vertex clustering (tests/_trianglemesh_clean_oracle.
py) against the literal vectors of upstream's own tests
(tests/golden/trianglemesh_clean_vectors.json) and against a second, literal
transcription of the legacy loops; and the binding of the new C ABI. No GPU."""
import json
import os
import re

import numpy as np
import pytest

import _trianglemesh_clean_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_CALLS = [
    "o3dmi_trianglemesh_remove_duplicated_vertices",
    "o3dmi_trianglemesh_remove_duplicated_triangles",
    "o3dmi_trianglemesh_remove_degenerate_triangles",
    "o3dmi_trianglemesh_compute_adjacency_list",
    "o3dmi_trianglemesh_filter_sharpen",
    "o3dmi_trianglemesh_filter_smooth_simple",
    "o3dmi_trianglemesh_filter_smooth_laplacian",
    "o3dmi_trianglemesh_filter_smooth_taubin",
    "o3dmi_trianglemesh_simplify_vertex_clustering",
]


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden",
                           "trianglemesh_clean_vectors.json")) as f:
        return json.load(f)


# ---- upstream's literals ------------------------------------------------------------
def test_adjacency_golden(gold):
    g = gold["adjacency"]
    sets = orc.adjacency_sets(g["triangles"], len(g["vertices"]))
    assert sets == [set(x) for x in g["lists"]]
    splits, nbrs = orc.adjacency_csr(g["triangles"], len(g["vertices"]))
    lists = [nbrs[splits[u]:splits[u + 1]].tolist() for u in range(5)]
    assert lists == g["lists"]  # ascending, as the goldens happen to be


def test_purge_golden(gold):
    """Upstream purges tm0 + tm1, two meshes drawn with the same seed: every
    vertex and every triangle twice. The expected mesh doubled the same way
    must come back as the expected mesh."""
    g = gold["purge"]
    p = np.array(g["vertices"])
    t = np.array(g["triangles"], np.int32)
    tn = np.array(g["triangle_normals"])
    n = len(p)
    p2, t2 = np.concatenate([p, p]), np.concatenate([t, t + n])
    vmask, tris, kept = orc.remove_duplicated_vertices(p2, t2)
    assert kept == n and vmask.tolist() == [1] * n + [0] * n
    assert tris.tolist() == np.concatenate([t, t]).tolist()
    tmask, tris = orc.remove_duplicated_triangles(tris)
    assert tmask.tolist() == [1] * len(t) + [0] * len(t)
    orc.expect_eq(np.concatenate([tn, tn])[tmask.astype(bool)], tn, 1e-6)
    dmask, tris = orc.remove_degenerate_triangles(tris)
    assert dmask.all() and tris.tolist() == g["triangles"]
    orc.expect_eq(p2[vmask.astype(bool)], g["vertices"], 1e-6)


def test_duplicated_triangle_key_is_legacys():
    rot = orc.rotate_triangle
    assert rot((0, 1, 2)) == rot((1, 2, 0)) == rot((2, 0, 1)) == (0, 1, 2)
    assert rot((0, 2, 1)) == (0, 2, 1) != rot((0, 1, 2))
    # the ties of the branch statements
    assert rot((5, 5, 3)) == (3, 5, 5) and rot((5, 3, 5)) == (3, 5, 5)
    assert rot((3, 5, 5)) == (3, 5, 5) and rot((5, 3, 3)) == (3, 3, 5)
    assert rot((4, 4, 4)) == (4, 4, 4)


def test_vertex_keys_by_value():
    p = np.array([[0.0, 1, 2], [-0.0, 1, 2], [np.nan, 0, 0], [np.nan, 0, 0],
                  [0.0, 1, 2]])
    vmask, tris, kept = orc.remove_duplicated_vertices(
        p, np.array([[0, 1, 4], [2, 3, 4]], np.int64))
    assert vmask.tolist() == [1, 0, 1, 1, 0] and kept == 3
    assert tris.tolist() == [[0, 0, 0], [1, 2, 0]]


@pytest.mark.parametrize("kind", ["sharpen", "simple", "laplacian", "taubin"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_filter_goldens(gold, kind, dtype):
    p = np.array(gold["star"]["vertices"], dtype)
    t = np.array(gold["star"]["triangles"], np.int32)
    for step in gold["filters"][kind]:
        p, _, _ = orc.run_filter(kind, p, None, None, t, step["iterations"],
                                 step["args"], orc.SCOPE_ALL)
        assert p.dtype == dtype
        orc.expect_eq(p, step["expected"], step["threshold"])


# ---- the legacy loops, transcribed a second time --------------------------------------
def _random_mesh(v, m, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((v, 3)), rng.standard_normal((v, 3)),
            rng.random((v, 3)), rng.integers(0, v, (m, 3)))


def _legacy_filter(kind, prev, tri, iterations, factors, scope):
    """geometry/TriangleMesh.cpp:167-440 with Python floats, the adjacency
    lists walked in ascending order; prev: [positions, normals, colors] as
    lists of rows. The attributes outside the scope keep their values and the
    weights use the current positions (the two stated differences)."""
    v = len(prev[0])
    adj = [sorted(s) for s in orc.adjacency_sets(tri, v)]
    wanted = [scope in (0, 3), scope in (0, 2), scope in (0, 1)]
    prev = [[list(r) for r in a] for a in prev]

    def plain():
        nxt = [[list(r) for r in a] for a in prev]
        for u in range(v):
            for a in range(3):
                if not wanted[a]:
                    continue
                s = [0.0, 0.0, 0.0]
                for nb in adj[u]:
                    s = [s[c] + prev[a][nb][c] for c in range(3)]
                n = float(len(adj[u]))
                for c in range(3):
                    x = prev[a][u][c]
                    if kind == "sharpen":
                        nxt[a][u][c] = x + factors[0] * (x * n - s[c])
                    else:
                        nxt[a][u][c] = (x + s[c]) / (1 + len(adj[u]))
        return nxt

    def laplacian(factor):
        nxt = [[list(r) for r in a] for a in prev]
        pos = prev[0]
        for a in range(3):
            if not wanted[a]:
                continue
            for u in range(v):
                total, s = 0.0, [0.0, 0.0, 0.0]
                for nb in adj[u]:
                    d = [pos[u][c] - pos[nb][c] for c in range(3)]
                    dist = float(np.sqrt((d[0] * d[0] + d[1] * d[1]) +
                                         d[2] * d[2]))
                    w = 1.0 / (dist + 1e-12)
                    total += w
                    s = [s[c] + w * prev[a][nb][c] for c in range(3)]
                if total > 0.0:
                    for c in range(3):
                        x = prev[a][u][c]
                        nxt[a][u][c] = x + factor * (s[c] / total - x)
        return nxt

    for _ in range(iterations):
        if kind in ("sharpen", "simple"):
            prev = plain()
        elif kind == "laplacian":
            prev = laplacian(factors[0])
        else:
            prev = laplacian(factors[0])
            prev = laplacian(factors[1])
    return [np.array(a) for a in prev]


@pytest.mark.parametrize("kind,factors", [
    ("sharpen", [0.3]), ("simple", []), ("laplacian", [0.5]),
    ("taubin", [0.5, -0.53])])
@pytest.mark.parametrize("scope", [0, 1, 2, 3])
def test_filters_equal_the_legacy_loops(kind, factors, scope):
    p, n, c, t = _random_mesh(60, 150, 11)
    t[7] = (6, 6, 7)      # a vertex that is its own neighbour
    t[t == 59] = 0        # vertex 59 is isolated
    want = _legacy_filter(kind, [p.tolist(), n.tolist(), c.tolist()], t, 2,
                          factors, scope)
    got = orc.run_filter(kind, p, n, c, t, 2, factors, scope)
    for a, b in zip(got, want):
        assert a.dtype == np.float64
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(got[0][59], p[59])


def test_clustering_equals_the_legacy_loops():
    """TriangleMeshSimplification.cpp:95-230 again: dictionaries keyed by the
    voxel, averages by numpy sums over ascending members."""
    p, n, c, t = _random_mesh(300, 700, 5)
    for voxel_size in (0.05, 0.7, 3.0):
        out = orc.simplify_vertex_clustering(p, n, c, t, voxel_size,
                                             orc.AVERAGE)
        lo = p.min(axis=0) - voxel_size * 0.5
        first, new = {}, []
        for i in range(len(p)):
            key = tuple(np.floor((p[i] - lo) / voxel_size).astype(int))
            new.append(first.setdefault(key, len(first)))
        assert out["new_index"].tolist() == new
        for k in range(len(first)):
            mem = [i for i in range(len(p)) if new[i] == k]
            s = np.zeros(3)
            for i in mem:
                s = s + p[i]
            assert np.array_equal(out["positions"][k], s / float(len(mem)))
        tris = out["triangles"].tolist()
        assert len(set(map(tuple, tris))) == len(tris)
        assert all(len({a, b, c}) == 3 and a == min(a, b, c)
                   for a, b, c in tris)


def test_quadric_meets_three_planes_exactly():
    """Planes x = 1, y = 2, z = 3 with power-of-two areas: every product and
    sum is exact, so the minimiser is (1, 2, 3) to the bit."""
    q = [0.0] * 12
    for axis, (d, w) in enumerate([(-1.0, 2.0), (-2.0, 0.5), (-3.0, 4.0)]):
        n = [0.0, 0.0, 0.0]
        n[axis] = 1.0
        for r in range(3):
            for s in range(3):
                q[3 * r + s] += (w * n[r]) * n[s]
            q[9 + r] += (w * d) * n[r]
    assert orc.quadric_minimum(q) == [1.0, 2.0, 3.0]
    assert orc.quadric_minimum([0.0] * 12) is None


# ---- the binding --------------------------------------------------------------------
def test_every_new_call_is_declared_and_bound():
    from open3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "o3d_mi355x_host.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_CALLS:
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\b%s\s*\(" % name, header), name


def test_python_mirror_has_the_family():
    import ast
    src = open(os.path.join(ROOT, "open3d_amd", "trianglemesh.py")).read()
    names = {n.name for n in ast.parse(src).body
             if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    for name in ("remove_duplicated_vertices", "remove_duplicated_triangles",
                 "remove_degenerate_triangles", "compute_adjacency_list",
                 "filter_sharpen", "filter_smooth_simple",
                 "filter_smooth_laplacian", "filter_smooth_taubin",
                 "simplify_vertex_clustering", "FilterScope",
                 "SimplificationContraction"):
        assert name in names, name
