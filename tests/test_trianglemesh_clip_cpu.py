"""The clip / slice oracle (tests/_trianglemesh_clip_oracle.py) alone, against
hand values that are exact in binary, upstream's two counts on the unit box,
and the invariants of the rules."""
import numpy as np

import _trianglemesh_clip_oracle as orc
import _trianglemesh_subdivide_oracle as sub

# TriangleMesh::CreateBox(1, 1, 1), restated as data
BOX_P = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1],
                  [0, 1, 0], [1, 1, 0], [0, 1, 1], [1, 1, 1]], np.float64)
BOX_T = np.array([[4, 7, 5], [4, 6, 7], [0, 2, 4], [2, 6, 4], [0, 1, 2],
                  [1, 3, 2], [1, 5, 7], [1, 7, 3], [2, 3, 7], [2, 7, 6],
                  [0, 4, 1], [1, 4, 5]], np.int64)
# the two-triangle quad of the subdivision test
QUAD_P = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]], np.float64)
QUAD_T = np.array([[0, 1, 2], [3, 2, 1]], np.int64)
TETRA_P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
TETRA_T = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)


def _counts(out):
    if "triangles" in out:
        return len(out["positions"]), len(out["triangles"])
    return len(out["positions"]), len(out["lines"])


def _loops(lines):
    """The closed loops of a line list in which every point has one line
    leaving and one entering it -> a list of point lists."""
    nxt = {int(a): int(b) for a, b in lines}
    assert len(nxt) == len(lines)
    assert sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, at = [], start
        while at not in seen:
            seen.add(at)
            loop.append(at)
            at = nxt[at]
        assert at == start
        loops.append(loop)
    return loops


def _area(p, t):
    p = p.astype(np.float64)
    cr = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    return 0.5 * np.sqrt((cr * cr).sum(axis=1)).sum()


# ---- upstream's two facts and the box cases ---------------------------------------
def test_clip_box_is_upstreams_test_clip_plane():
    out = orc.clip_plane(BOX_P, BOX_T, (0.5, 0, 0), (1, 0, 0))
    assert _counts(out) == (12, 14)
    assert np.array_equal(out["positions"][:4], BOX_P[[1, 3, 5, 7]])
    assert (out["positions"][4:, 0] == 0.5).all()
    assert (out["vertex_t"][4:] == 0.5).all()
    assert (out["positions"][:, 0] >= 0.5).all()


def test_slice_box_is_upstreams_test_slice_plane():
    out = orc.slice_plane(BOX_P, BOX_T, (0, 0.5, 0), (1, 1, 1),
                          (-0.1, 0, 0.1))
    assert _counts(out) == (9, 9)
    assert out["line_contour"].tolist() == [0] * 3 + [1] * 3 + [2] * 3
    assert len(_loops(out["lines"])) == 3


def test_clip_box_touching_and_whole():
    for point, normal, want in (
            ((1, 0, 0), (1, 0, 0), (4, 2)),     # the face x = 1 stays
            ((0, 0, 0), (-1, 0, 0), (4, 2)),    # the face x = 0 stays
            ((0, 0, 0), (1, 1, 0), (8, 12)),    # the whole box
            ((0, 0, 0), (-1, -1, -1), (0, 0))):  # touches one corner
        out = orc.clip_plane(BOX_P, BOX_T, point, normal)
        assert _counts(out) == want, (point, normal)
    whole = orc.clip_plane(BOX_P, BOX_T, (0, 0, 0), (1, 1, 0))
    assert np.array_equal(whole["positions"], BOX_P)
    assert np.array_equal(whole["triangles"], BOX_T)
    assert whole["triangle_source"].tolist() == list(range(12))
    face = orc.clip_plane(BOX_P, BOX_T, (1, 0, 0), (1, 0, 0))
    assert np.array_equal(face["positions"], BOX_P[[1, 3, 5, 7]])
    assert face["triangle_source"].tolist() == [6, 7]


def test_slice_box_in_plane_faces():
    out = orc.slice_plane(BOX_P, BOX_T, (1, 0, 0), (1, 0, 0))
    assert _counts(out) == (4, 4)
    assert len(_loops(out["lines"])) == 1
    assert (out["point_source"][:, 0] == out["point_source"][:, 1]).all()
    assert sorted(out["point_source"][:, 0].tolist()) == [1, 3, 5, 7]
    assert _counts(orc.slice_plane(BOX_P, BOX_T, (0, 0, 0), (1, 0, 0))) == \
        (0, 0)


def test_slice_box_through_four_vertices_and_one_edge_point():
    out = orc.slice_plane(BOX_P, BOX_T, (0, 0, 0), (1, -1, 0))
    assert _counts(out) == (5, 5)
    (loop,) = _loops(out["lines"])
    assert len(loop) == 5
    src = out["point_source"]
    vertex_points = sorted(int(a) for a, b in src if a == b)
    assert vertex_points == [0, 2, 5, 7]
    (edge,) = [i for i, (a, b) in enumerate(src) if a != b]
    assert out["positions"][edge].tolist() == [0.5, 0.5, 0]
    assert src[edge].tolist() == [1, 4] and out["point_t"][edge] == 0.5


# ---- numbering, by hand -----------------------------------------------------------
def test_clip_numbers_a_shared_edge_by_its_lowest_slot():
    """x >= 1 on the quad. Triangle 0 = (0, 1, 2) has 1 inside: rotated (1, 2,
    0), piece (1, ab, ca) with ab on slot 1, ca on slot 0. Triangle 1 = (3, 2,
    1) has 2 outside: rotated (1, 3, 2), pieces (1, 3, bc), (1, bc, ca) with bc
    on slot 3 and ca, the shared edge again, on slot 4. Old vertices 1, 3 ->
    0, 1; edges by lowest slot: (0, 1) slot 0 -> 2, (1, 2) slot 1 -> 3, (2, 3)
    slot 3 -> 4."""
    out = orc.clip_plane(QUAD_P, QUAD_T, (1, 0, 0), (1, 0, 0))
    assert out["triangles"].tolist() == [[0, 3, 2], [0, 1, 4], [0, 4, 3]]
    assert out["triangle_source"].tolist() == [0, 1, 1]
    assert out["vertex_source"].tolist() == [[1, 1], [3, 3], [0, 1], [1, 2],
                                             [2, 3]]
    assert out["vertex_t"].tolist() == [0, 0, .5, .5, .5]
    assert out["positions"].tolist() == [[2, 0, 0], [2, 2, 0], [1, 0, 0],
                                         [1, 1, 0], [1, 2, 0]]


def test_slice_numbers_points_by_the_lowest_slot_of_their_uses():
    """The same cut as lines: triangle 0 gives (ab, ca) = ((1, 2) on slot 1,
    (0, 1) on slot 0), triangle 1 gives (bc, ca) = ((2, 3) on slot 3, (1, 2) on
    slot 4): points (0, 1) -> 0, (1, 2) -> 1, (2, 3) -> 2."""
    out = orc.slice_plane(QUAD_P, QUAD_T, (1, 0, 0), (1, 0, 0))
    assert out["lines"].tolist() == [[1, 0], [2, 1]]
    assert out["line_triangle"].tolist() == [0, 1]
    assert out["point_source"].tolist() == [[0, 1], [1, 2], [2, 3]]
    assert out["positions"].tolist() == [[1, 0, 0], [1, 1, 0], [1, 2, 0]]


def test_unnormalised_normal_scales_the_contour_value():
    a = orc.slice_plane(QUAD_P, QUAD_T, (0, 0, 0), (1, 0, 0), (1.0,))
    b = orc.slice_plane(QUAD_P, QUAD_T, (0, 0, 0), (2, 0, 0), (2.0,))
    c = orc.slice_plane(QUAD_P, QUAD_T, (0, 0, 0), (2, 0, 0), (1.0,))
    assert np.array_equal(a["positions"], b["positions"])
    assert (c["positions"][:, 0] == 0.5).all()


def test_degenerate_and_doubled_triangles():
    p = np.array([[1, 0, 0], [-1, 0, 0], [1, 1, 0], [-1, 1, 0]], np.float64)
    # (a, a, b) across the plane and wholly inside: both vanish
    for t in ([[0, 0, 1]], [[0, 1, 1]], [[0, 0, 2]], [[0, 0, 0]]):
        out = orc.clip_plane(p, t, (0, 0, 0), (1, 0, 0))
        assert _counts(out) == (0, 0), t
        assert _counts(orc.slice_plane(p, t, (0, 0, 0), (1, 0, 0))) == (0, 0)
    # a doubled triangle: both copies stay and share their cut vertices
    out = orc.clip_plane(p, [[0, 1, 2], [0, 1, 2]], (0, 0, 0), (1, 0, 0))
    assert _counts(out) == (4, 4)
    assert out["triangles"][:2].tolist() == out["triangles"][2:].tolist()
    assert out["triangle_source"].tolist() == [0, 0, 1, 1]
    lines = orc.slice_plane(p, [[0, 1, 2], [0, 1, 2]], (0, 0, 0), (1, 0, 0))
    assert _counts(lines) == (2, 2)
    assert lines["lines"][0].tolist() == lines["lines"][1].tolist()


def test_unreferenced_and_outside_vertices_disappear():
    p = np.concatenate([[[5., 6., 7.]], QUAD_P])
    out = orc.clip_plane(p, QUAD_T + 1, (1, 0, 0), (1, 0, 0))
    ref = orc.clip_plane(QUAD_P, QUAD_T, (1, 0, 0), (1, 0, 0))
    assert np.array_equal(out["positions"], ref["positions"])
    assert np.array_equal(out["triangles"], ref["triangles"])
    assert np.array_equal(out["vertex_source"], ref["vertex_source"] + 1)


def test_touching_from_below_vanishes_and_in_plane_stays():
    p = np.array([[0, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 1], [1, 0, 0],
                  [-1, 1, 0]], np.float64)
    at, n = (0, 0, 0), (1, 0, 0)
    assert _counts(orc.clip_plane(p, [[0, 2, 5]], at, n)) == (0, 0)  # a vertex
    assert _counts(orc.clip_plane(p, [[0, 1, 2]], at, n)) == (0, 0)  # an edge
    assert _counts(orc.clip_plane(p, [[0, 1, 3]], at, n)) == (3, 1)  # in plane
    assert _counts(orc.slice_plane(p, [[0, 2, 5]], at, n)) == (0, 0)
    # one vertex on the plane, one above, one below: the cut goes through the
    # vertex and makes one new point, on the opposite edge
    out = orc.clip_plane(p, [[1, 4, 2]], at, n)
    assert _counts(out) == (3, 1)
    assert out["vertex_source"].tolist() == [[1, 1], [4, 4], [2, 4]]
    # slice: the in-plane edge is emitted by the triangle whose third vertex
    # is below, not by the one above, and not by the in-plane triangle
    assert _counts(orc.slice_plane(p, [[0, 1, 2]], at, n)) == (2, 1)
    assert _counts(orc.slice_plane(p, [[0, 1, 4]], at, n)) == (0, 0)
    assert _counts(orc.slice_plane(p, [[0, 1, 3]], at, n)) == (0, 0)


def test_slice_edge_points_have_clips_bits():
    rng = np.random.default_rng(5)
    p, _, _, t = sub.subdivide_midpoint(TETRA_P, TETRA_T, 2)
    p = (p + 0.01 * rng.standard_normal(p.shape)).astype(np.float32)
    nrm = rng.standard_normal(p.shape).astype(np.float32)
    at, n = (0.21, 0.2, 0.3), (0.3, -0.5, 0.8)
    clip = orc.clip_plane(p, t, at, n, normals=nrm)
    cut = orc.slice_plane(p, t, at, n, normals=nrm)
    by_edge = {tuple(e): i for i, e in enumerate(clip["vertex_source"])}
    assert len(cut["positions"]) > 8
    for i, e in enumerate(cut["point_source"]):
        j = by_edge[tuple(e)]
        assert e[0] != e[1]
        for name in ("positions", "normals"):
            assert cut[name][i].tobytes() == clip[name][j].tobytes()
        assert cut["point_t"][i] == clip["vertex_t"][j]


def test_invariants_on_the_subdivided_tetrahedron():
    p, _, _, t = sub.subdivide_midpoint(TETRA_P, TETRA_T, 3)
    assert t.shape == (256, 3)
    at, n = (0.23, 0.19, 0.31), (0.3, -0.5, 0.8)
    s = orc.signed_values(p, at, n)
    assert (s != 0).all()  # the plane goes through no vertex
    cut = orc.slice_plane(p, t, at, n)
    loops = _loops(cut["lines"])  # one line leaving, one entering every point
    assert len(loops) == 1 and len(loops[0]) == len(cut["positions"]) > 0
    above = orc.clip_plane(p, t, at, n)
    below = orc.clip_plane(p, t, at, [-x for x in n])
    total = _area(p, t)
    parts = _area(above["positions"], above["triangles"]) + \
        _area(below["positions"], below["triangles"])
    assert abs(parts - total) <= 1e-10 * total
    assert len(above["triangles"]) > 0 and len(below["triangles"]) > 0
    # every cut vertex is shared by both halves, bit for bit
    new_a = above["positions"][above["vertex_t"] != 0]
    new_b = below["positions"][below["vertex_t"] != 0]
    assert sorted(map(bytes, new_a)) == sorted(map(bytes, new_b))
