"""The numpy restatement of the TriangleMesh operators against the literal
inputs and expected outputs of upstream's own tests
(tests/golden/trianglemesh_vectors.json). No GPU."""
import numpy as np
import pytest

import _trianglemesh_oracle as oracle


@pytest.fixture(scope="module")
def gold():
    return oracle.golden()


@pytest.mark.parametrize("name", ["cluster_boxes", "cluster_pairs"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_legacy_cluster_goldens(gold, name, dtype):
    g = gold[name]
    labels, counts, areas = oracle.cluster_connected_triangles(
        np.array(g["vertices"], dtype), g["triangles"])
    assert labels.tolist() == g["labels"]
    assert counts.tolist() == g["n_triangles"]
    # Float64: upstream's literals exactly (its EXPECT_EQ); Float32 positions:
    # the literals rounded to float32 and widened
    want = np.array(g["areas"], dtype).astype(np.float64)
    assert areas.tolist() == want.tolist()


def test_non_manifold_edges_golden(gold):
    g = gold["non_manifold"]
    closed = oracle.non_manifold_edges(g["triangles"], False)
    assert sorted(map(tuple, closed.tolist())) == \
        sorted(map(tuple, g["edges_no_boundary"]))
    assert closed.tolist() == sorted(closed.tolist())  # ascending (lo, hi)
    ones = set(map(tuple, g["multiplicity_one"]))
    boundary = oracle.non_manifold_edges(g["triangles"], True)
    assert set(map(tuple, boundary.tolist())) == \
        set(map(tuple, g["edges_no_boundary"])) - ones
    edges = oracle.edge_map(g["triangles"])
    assert len(edges[(6, 6)]) == 1 and len(edges[(6, 7)]) == 4
    assert all(len(edges[e]) == 1 for e in ones)


def test_select_faces_by_mask_golden(gold):
    box, g = gold["box"], gold["select_faces_by_mask"]
    vmask, tris = oracle.select_faces_by_mask(box["triangles"], 8, g["mask"])
    want = g["expected"]
    assert tris.tolist() == want["triangles"]
    for name in ("vertices", "vertex_colors", "vertex_labels"):
        assert np.array(box[name])[vmask].tolist() == \
            np.array(want[name], float).tolist()
    assert np.array(box["triangle_labels"])[np.array(g["mask"], bool)] \
        .tolist() == want["triangle_labels"]


@pytest.mark.parametrize("case", ["basic", "duplicate", "negative",
                                  "no_triangles"])
def test_select_by_index_golden(gold, case):
    box, g = gold["box"], gold["select_by_index"][case]
    vmask, tmask, tris, ignored = oracle.select_by_index(box["triangles"], 8,
                                                         g["indices"])
    want = g["expected"]
    assert tris.tolist() == want["triangles"]
    assert ignored == g.get("ignored", 0)
    assert np.array(box["vertices"])[vmask].tolist() == \
        np.array(want["vertices"], float).tolist()
    assert np.array(box["vertex_colors"])[vmask].tolist() == \
        want["vertex_colors"]
    assert np.array(box["vertex_labels"])[vmask].tolist() == \
        want["vertex_labels"]
    if "triangle_mask" in want:
        assert tmask.astype(int).tolist() == want["triangle_mask"]
    else:
        assert not tmask.any()


def test_remove_unreferenced_vertices_golden(gold):
    g = gold["remove_unreferenced_vertices"]
    vmask, tris = oracle.remove_unreferenced_vertices(g["triangles"],
                                                      len(g["vertices"]))
    assert vmask.astype(int).tolist() == g["vertex_mask"]
    # the triangles renumbered by upstream's literal vertex mask: an 18-vertex
    # list that names every vertex
    assert tris.tolist() == g["expected_triangles"]
    assert sorted(set(tris.reshape(-1).tolist())) == list(range(18))


def test_elementwise_statements():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    t = [[0, 1, 2]]
    assert oracle.triangle_normals(p, t).tolist() == [[0.0, 0.0, 2.0]]
    assert oracle.triangle_areas(p, t).tolist() == [1.0]
    assert oracle.surface_area(p, t * 1025) == 1025.0
    n = np.array([[np.nan, 1, 2], [3, np.nan, 4], [0, 0, 0], [0, 3, 4]],
                 np.float32)
    out = oracle.normalize_normals(n)
    assert np.isnan(out[0, 0]) and out[0, 1:].tolist() == [1.0, 2.0]
    # only y is NaN: the norm is NaN, `norm > 0` fails, the row is stored as is
    assert out[1, 0] == 3 and np.isnan(out[1, 1]) and out[1, 2] == 4
    assert out[2].tolist() == [0.0, 0.0, 0.0]
    assert out[3].tolist() == [0.0, np.float32(3) / np.float32(5),
                               np.float32(4) / np.float32(5)]


def test_vertex_normal_sum_is_sequential():
    tn = np.array([[1e3, 0, 0], [1e-3, 0, 0], [-1e3, 0, 0]], np.float32)
    t = [[0, 1, 2], [0, 0, 3], [0, 4, 5]]
    out = oracle.vertex_normals(t, tn, 7)
    seq = np.float32(0)
    for x in (tn[0, 0], tn[1, 0], tn[1, 0], tn[2, 0]):
        seq = seq + x
    assert out[0, 0] == seq and out[6].tolist() == [0.0, 0.0, 0.0]
