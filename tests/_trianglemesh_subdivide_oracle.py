"""Restatement of legacy SubdivideMidpoint / SubdivideLoop (geometry/
TriangleMeshSubdivide.cpp) that follows upstream's loops literally: a dict for
new_verts, the per-triangle walk, a dict of sets for edge_to_triangles and a
list of sets for vertex_neighbours. Where upstream iterates an unordered_set,
the set is iterated in ascending order (the pinned order; equal to rounding).

Arithmetic is Python float (IEEE float64, one rounding per operation, nothing
contracted). Positions, normals and colours go through the same statements
component by component, so a vertex is one row of 3 k floats: the attributes
side by side. A Float32 mesh is widened on load and narrowed once at the end;
narrow_each_iteration=True narrows after every iteration instead (what the
device must NOT do).

subdivide_loop(..., upstream_unreferenced=True) keeps upstream's statements
for a vertex without neighbours (beta = 3 / (8 * 0) = inf, alpha = 1 - 0 * inf
= NaN); the default copies such a vertex, as the device does.
"""
import numpy as np


def _load(positions, normals, colors):
    given = [a for a in (positions, normals, colors) if a is not None]
    rows = np.concatenate([np.asarray(a, np.float64) for a in given], axis=1)
    return [list(map(float, r)) for r in rows], len(given)


def _through(rows, dtype):
    if not rows:
        return rows
    a = np.asarray(rows, np.float64).astype(dtype).astype(np.float64)
    return [list(map(float, r)) for r in a]


def _store(rows, k, positions, normals, colors, triangles, index_dtype):
    a = np.asarray(rows, np.float64).reshape(len(rows), 3 * k)
    a = a.astype(positions.dtype)
    out, col = [], 0
    for given in (positions, normals, colors):
        if given is None:
            out.append(None)
        else:
            out.append(np.ascontiguousarray(a[:, col:col + 3]))
            col += 3
    tri = np.asarray(triangles, index_dtype).reshape(len(triangles), 3)
    return out[0], out[1], out[2], tri


def _ordered(a, b):
    return (min(a, b), max(a, b))


def subdivide_midpoint(positions, triangles, number_of_iterations,
                       normals=None, colors=None,
                       narrow_each_iteration=False):
    """-> (positions, normals, colors, triangles) by :18-94."""
    verts, k = _load(positions, normals, colors)
    tris = [tuple(int(i) for i in t) for t in triangles]

    def subdivide_edge(new_verts, vidx0, vidx1):
        lo, hi = min(vidx0, vidx1), max(vidx0, vidx1)
        edge = (lo, hi)
        if edge not in new_verts:
            verts.append([0.5 * (a + b) for a, b in zip(verts[lo], verts[hi])])
            new_verts[edge] = len(verts) - 1
        return new_verts[edge]

    for _ in range(number_of_iterations):
        new_verts = {}
        new_tris = [None] * (4 * len(tris))
        for tidx, (v0, v1, v2) in enumerate(tris):
            v01 = subdivide_edge(new_verts, v0, v1)
            v12 = subdivide_edge(new_verts, v1, v2)
            v20 = subdivide_edge(new_verts, v2, v0)
            new_tris[4 * tidx + 0] = (v0, v01, v20)
            new_tris[4 * tidx + 1] = (v01, v1, v12)
            new_tris[4 * tidx + 2] = (v12, v2, v20)
            new_tris[4 * tidx + 3] = (v01, v12, v20)
        tris = new_tris
        if narrow_each_iteration:
            verts = _through(verts, positions.dtype)
    return _store(verts, k, positions, normals, colors, tris,
                  np.asarray(triangles).dtype)


def edge_multiplicities(triangles):
    """{(lo, hi): number of distinct triangles} by :270-279."""
    edge_to_triangles = {}
    for tidx, (a, b, c) in enumerate(triangles):
        for e in (_ordered(a, b), _ordered(b, c), _ordered(c, a)):
            edge_to_triangles.setdefault(e, set()).add(tidx)
    return {e: len(s) for e, s in edge_to_triangles.items()}


def subdivide_loop(positions, triangles, number_of_iterations, normals=None,
                   colors=None, upstream_unreferenced=False,
                   narrow_each_iteration=False):
    """-> (positions, normals, colors, triangles) by :96-357."""
    old_verts, k = _load(positions, normals, colors)
    old_tris = [tuple(int(i) for i in t) for t in triangles]

    def update_vertex(vidx, new_verts_rows, nbs, edge_to_triangles):
        boundary_nbs = set()
        for nb in sorted(nbs):
            if len(edge_to_triangles[_ordered(vidx, nb)]) == 1:
                boundary_nbs.add(nb)
        if not nbs and not upstream_unreferenced:
            new_verts_rows[vidx] = list(old_verts[vidx])
            return
        if len(boundary_nbs) >= 2:
            beta = 1. / 8.
            alpha = 1. - len(boundary_nbs) * beta
        elif len(nbs) == 3:
            beta = 3. / 16.
            alpha = 1. - len(nbs) * beta
        else:
            beta = 3. / (8. * len(nbs)) if nbs else float("inf")
            alpha = 1. - len(nbs) * beta
        row = [alpha * x for x in old_verts[vidx]]
        chosen = boundary_nbs if len(boundary_nbs) >= 2 else nbs
        for nb in sorted(chosen):
            row = [r + beta * x for r, x in zip(row, old_verts[nb])]
        new_verts_rows[vidx] = row

    def subdivide_edge(vidx0, vidx1, new_verts_rows, new_verts,
                       edge_to_triangles):
        edge = _ordered(vidx0, vidx1)
        if edge in new_verts:
            return new_verts[edge]
        row = [a + b for a, b in zip(old_verts[vidx0], old_verts[vidx1])]
        edge_triangles = edge_to_triangles[edge]
        if len(edge_triangles) < 2:
            row = [x * 0.5 for x in row]
        else:
            row = [x * (3. / 8.) for x in row]
            scale = 1. / (4. * len(edge_triangles))
            for tidx in sorted(edge_triangles):
                tria = old_tris[tidx]
                vidx2 = tria[0] if (tria[0] != vidx0 and tria[0] != vidx1) \
                    else (tria[1] if (tria[1] != vidx0 and tria[1] != vidx1)
                          else tria[2])
                row = [r + scale * x for r, x in zip(row, old_verts[vidx2])]
        vidx01 = len(old_verts) + len(new_verts)
        new_verts_rows[vidx01] = row
        new_verts[edge] = vidx01
        return vidx01

    def insert_triangle(tidx, v0, v1, v2, tris, edge_to_triangles,
                        vertex_neighbours):
        tris[tidx] = (v0, v1, v2)
        edge_to_triangles.setdefault(_ordered(v0, v1), set()).add(tidx)
        edge_to_triangles.setdefault(_ordered(v1, v2), set()).add(tidx)
        edge_to_triangles.setdefault(_ordered(v2, v0), set()).add(tidx)
        vertex_neighbours[v0].update((v1, v2))
        vertex_neighbours[v1].update((v0, v2))
        vertex_neighbours[v2].update((v0, v1))

    edge_to_triangles = {}
    vertex_neighbours = [set() for _ in old_verts]
    scratch = [None] * len(old_tris)
    for tidx, (a, b, c) in enumerate(old_tris):
        insert_triangle(tidx, a, b, c, scratch, edge_to_triangles,
                        vertex_neighbours)

    for _ in range(number_of_iterations):
        n_new_vertices = len(old_verts) + len(edge_to_triangles)
        new_rows = [None] * n_new_vertices
        new_tris = [None] * (4 * len(old_tris))
        new_verts = {}
        new_edge_to_triangles = {}
        new_vertex_neighbours = [set() for _ in range(n_new_vertices)]
        for vidx in range(len(old_verts)):
            update_vertex(vidx, new_rows, vertex_neighbours[vidx],
                          edge_to_triangles)
        for tidx, (v0, v1, v2) in enumerate(old_tris):
            v01 = subdivide_edge(v0, v1, new_rows, new_verts,
                                 edge_to_triangles)
            v12 = subdivide_edge(v1, v2, new_rows, new_verts,
                                 edge_to_triangles)
            v20 = subdivide_edge(v2, v0, new_rows, new_verts,
                                 edge_to_triangles)
            insert_triangle(4 * tidx + 0, v0, v01, v20, new_tris,
                            new_edge_to_triangles, new_vertex_neighbours)
            insert_triangle(4 * tidx + 1, v01, v1, v12, new_tris,
                            new_edge_to_triangles, new_vertex_neighbours)
            insert_triangle(4 * tidx + 2, v12, v2, v20, new_tris,
                            new_edge_to_triangles, new_vertex_neighbours)
            insert_triangle(4 * tidx + 3, v01, v12, v20, new_tris,
                            new_edge_to_triangles, new_vertex_neighbours)
        old_verts, old_tris = new_rows, new_tris
        edge_to_triangles = new_edge_to_triangles
        vertex_neighbours = new_vertex_neighbours
        if narrow_each_iteration:
            old_verts = _through(old_verts, positions.dtype)
    return _store(old_verts, k, positions, normals, colors, old_tris,
                  np.asarray(triangles).dtype)
