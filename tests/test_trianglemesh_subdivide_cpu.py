"""The subdivision oracle (tests/_trianglemesh_subdivide_oracle.py) against
hand values that are exact in binary, hence independent of any pinned order,
and against the counting rules the device restates."""
import numpy as np

import _trianglemesh_subdivide_oracle as orc

TRIANGLE_P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
TRIANGLE_T = np.array([[0, 1, 2]], np.int32)
TETRA_P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
TETRA_T = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)


def test_loop_single_triangle_hand_values():
    p, n, c, t = orc.subdivide_loop(TRIANGLE_P, TRIANGLE_T, 1)
    assert n is None and c is None
    assert np.array_equal(p, np.array([
        [.125, .125, 0], [.75, .125, 0], [.125, .75, 0],
        [.5, 0, 0], [.5, .5, 0], [0, .5, 0]]))
    assert t.dtype == np.int32
    assert t.tolist() == [[0, 3, 5], [3, 1, 4], [4, 2, 5], [3, 4, 5]]


def test_loop_tetrahedron_hand_values_and_counts():
    p, _, _, t = orc.subdivide_loop(TETRA_P, TETRA_T, 1)
    assert p.shape == (10, 3) and t.shape == (16, 3)
    assert p[0].tolist() == [.1875, .1875, .1875]
    assert p[4].tolist() == [.125, .375, .125]  # the edge (0, 2)
    p3, _, _, t3 = orc.subdivide_loop(TETRA_P, TETRA_T, 3)
    assert p3.shape == (130, 3) and t3.shape == (256, 3)
    pm, _, _, tm = orc.subdivide_midpoint(TETRA_P, TETRA_T, 3)
    assert pm.shape == (130, 3) and tm.shape == (256, 3)


def test_midpoint_numbers_a_shared_edge_at_its_first_encounter():
    p = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]], np.float64)
    t = np.array([[0, 1, 2], [3, 2, 1]], np.int64)
    q, _, _, u = orc.subdivide_midpoint(p, t, 1)
    # walk: (0,1) -> 4, (1,2) -> 5, (2,0) -> 6, then (3,2) -> 7, (2,1) is 5
    # again, (1,3) -> 8
    assert u.dtype == np.int64
    assert u.tolist() == [[0, 4, 6], [4, 1, 5], [5, 2, 6], [4, 5, 6],
                          [3, 7, 8], [7, 2, 5], [5, 1, 8], [7, 5, 8]]
    assert q[4:].tolist() == [[1, 0, 0], [1, 1, 0], [0, 1, 0], [1, 2, 0],
                              [2, 1, 0]]
    assert np.array_equal(q[:4], p)


def test_degenerate_triangle_count_follows_the_walk():
    p = np.array([[0, 0, 0], [1, 0, 0]], np.float64)
    t = np.array([[0, 0, 1]], np.int32)
    q, _, _, u = orc.subdivide_midpoint(p, t, 1)
    # edges (0,0) -> 2, (0,1) -> 3, (1,0) again: E = 2, not 2 E + 3 M
    assert q.shape == (4, 3)
    assert u.tolist() == [[0, 2, 3], [2, 0, 3], [3, 1, 3], [2, 3, 3]]
    assert q[2].tolist() == [0, 0, 0] and q[3].tolist() == [.5, 0, 0]
    ql, _, _, ul = orc.subdivide_loop(p, t, 1)
    assert ql.shape == (4, 3) and np.array_equal(ul, u)


def test_unreferenced_vertex_switch():
    p = np.concatenate([TRIANGLE_P, [[5., 6., 7.]]])
    ours, _, _, _ = orc.subdivide_loop(p, TRIANGLE_T, 1)
    theirs, _, _, _ = orc.subdivide_loop(p, TRIANGLE_T, 1,
                                         upstream_unreferenced=True)
    assert ours[3].tolist() == [5., 6., 7.]
    assert np.isnan(theirs[3]).all()
    keep = [0, 1, 2, 4, 5, 6]
    assert np.array_equal(ours[keep], theirs[keep])
    assert not np.isnan(ours).any()


def test_multiplicity_counts_distinct_triangles():
    assert orc.edge_multiplicities([(0, 0, 1)]) == {(0, 0): 1, (0, 1): 1}
    assert orc.edge_multiplicities([(0, 1, 2), (0, 1, 2)]) == \
        {(0, 1): 2, (1, 2): 2, (0, 2): 2}
    # hence the doubled triangle is interior everywhere: its new vertices use
    # the 3/8 rule with both copies' opposite vertex
    p, _, _, _ = orc.subdivide_loop(TRIANGLE_P, np.array(
        [[0, 1, 2], [0, 1, 2]], np.int32), 1)
    assert p[3].tolist() == [.375, .25, 0]  # 3/8 (1,0,0) + 2/8 (0,1,0)


def test_attributes_ride_along_and_float32_is_narrowed_once():
    rng = np.random.default_rng(5)
    p = rng.standard_normal((4, 3)).astype(np.float32)
    n = rng.standard_normal((4, 3)).astype(np.float32)
    c = rng.random((4, 3)).astype(np.float32)
    q, m, d, _ = orc.subdivide_loop(p, TETRA_T, 2, normals=n, colors=c)
    assert q.dtype == m.dtype == d.dtype == np.float32
    # every attribute goes through the positions' statements
    q2, _, _, _ = orc.subdivide_loop(n, TETRA_T, 2)
    assert np.array_equal(m, q2)
    # the float64 result of the widened mesh, narrowed, is the same thing
    q3, _, _, _ = orc.subdivide_loop(p.astype(np.float64), TETRA_T, 2)
    assert np.array_equal(q, q3.astype(np.float32))
