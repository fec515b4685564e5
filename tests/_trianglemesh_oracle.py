"""Plain numpy restatement of the TriangleMesh operators: upstream's statements
in upstream's order (t/geometry/kernel/TriangleMeshImpl.h, TriangleMeshCPU.cpp,
t/geometry/TriangleMesh.cpp:1175-1452 and 1826-1864, legacy geometry/
TriangleMesh.cpp:1459-1528), with sequential Python loops wherever the order
of additions matters and arithmetic kept in the tensors' dtype."""
import collections
import json
import os

import numpy as np

RUN = 512  # values added in index order per run of the fixed float64 trees

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "trianglemesh_vectors.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _quiet(fn):
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    return wrapped


@_quiet
def cross(positions, triangles):
    """cross_3x1(p2 - p1, p3 - p1) per triangle, in the position dtype."""
    p = np.asarray(positions)
    t = np.asarray(triangles, np.int64)
    v01 = p[t[:, 1]] - p[t[:, 0]]
    v02 = p[t[:, 2]] - p[t[:, 0]]
    c = np.empty((t.shape[0], 3), p.dtype)
    c[:, 0] = v01[:, 1] * v02[:, 2] - v01[:, 2] * v02[:, 1]
    c[:, 1] = v01[:, 2] * v02[:, 0] - v01[:, 0] * v02[:, 2]
    c[:, 2] = v01[:, 0] * v02[:, 1] - v01[:, 1] * v02[:, 0]
    return c


triangle_normals = cross


@_quiet
def triangle_areas(positions, triangles):
    c = cross(positions, triangles)
    half = c.dtype.type(0.5)
    return half * np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) +
                          c[:, 2] * c[:, 2])


def tree_sum(values):
    """Float64 sum in the fixed tree: runs of RUN values in index order, the
    run sums likewise, until one value is left."""
    level = [float(x) for x in np.asarray(values, np.float64)]
    if not level:
        return 0.0
    while True:
        sums = []
        for r in range(0, len(level), RUN):
            s = np.float64(level[r])
            for x in level[r + 1:r + RUN]:
                s = s + np.float64(x)
            sums.append(s)
        level = sums
        if len(level) == 1:
            return float(level[0])


def surface_area(positions, triangles):
    return tree_sum(triangle_areas(positions, triangles))


@_quiet
def normalize_normals(normals):
    """The mesh rule: a row whose x is NaN is not stored to."""
    n = np.array(normals, copy=True)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    norm = np.sqrt((x * x + y * y) + z * z)
    store = ~np.isnan(x)
    div = store & (norm > 0)
    out = n.copy()
    for c in range(3):
        out[div, c] = n[div, c] / norm[div]
    return out


def vertex_normals(triangles, tri_normals, v):
    """ComputeVertexNormalsCPU: one triangle after the other."""
    tn = np.asarray(tri_normals)
    out = np.zeros((v, 3), tn.dtype)
    with np.errstate(all="ignore"):
        for i, tri in enumerate(np.asarray(triangles, np.int64)):
            for u in tri:
                out[u] = out[u] + tn[i]
    return out


def edge_map(triangles):
    """GetEdgeToTrianglesMap by edge slot: (lo, hi) -> the triangles of its
    slots (a triangle appears once per slot)."""
    edges = collections.OrderedDict()
    for t, (a, b, c) in enumerate(np.asarray(triangles, np.int64).tolist()):
        for x, y in ((a, b), (b, c), (c, a)):
            edges.setdefault((min(x, y), max(x, y)), []).append(t)
    return edges


def non_manifold_edges(triangles, allow_boundary_edges=True):
    """In ascending (lo, hi) order."""
    out = []
    for edge, tris in sorted(edge_map(triangles).items()):
        n = len(tris)
        if (allow_boundary_edges and (n < 1 or n > 2)) or \
                (not allow_boundary_edges and n != 2):
            out.append(edge)
    return np.array(out, np.int64).reshape(-1, 2)


def legacy_triangle_area(positions, tri):
    p = np.asarray(positions, np.float64)
    x = p[tri[0]] - p[tri[1]]
    y = p[tri[0]] - p[tri[2]]
    c0 = x[1] * y[2] - x[2] * y[1]
    c1 = x[2] * y[0] - x[0] * y[2]
    c2 = x[0] * y[1] - x[1] * y[0]
    with np.errstate(all="ignore"):
        return np.float64(0.5) * np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)


def cluster_connected_triangles(positions, triangles, areas=None):
    """The legacy breadth-first loop -> (labels, n_triangles, areas); a
    cluster's area is the two-level sum over its triangles in ascending
    index. `areas`: per-triangle float64 areas instead of the positions'."""
    tris = np.asarray(triangles, np.int64)
    m = tris.shape[0]
    edges = edge_map(tris)
    adjacency = [set() for _ in range(m)]
    for t, (a, b, c) in enumerate(tris.tolist()):
        for x, y in ((a, b), (a, c), (b, c)):
            adjacency[t].update(edges[(min(x, y), max(x, y))])
    labels = np.full(m, -1, np.int32)
    counts = []
    for seed in range(m):
        if labels[seed] != -1:
            continue
        c = len(counts)
        queue = collections.deque([seed])
        labels[seed] = c
        n = 0
        while queue:
            t = queue.popleft()
            n += 1
            for nb in adjacency[t]:
                if labels[nb] == -1:
                    queue.append(nb)
                    labels[nb] = c
        counts.append(n)
    if areas is None:
        areas = [legacy_triangle_area(positions, tris[t]) for t in range(m)]
    areas = np.asarray(areas, np.float64)
    cluster_areas = []
    for c in range(len(counts)):
        members = areas[labels == c]  # ascending triangle index
        runs = []
        for r in range(0, len(members), RUN):
            s = members[r]
            for x in members[r + 1:r + RUN]:
                s = s + x
            runs.append(s)
        s = runs[0]
        for x in runs[1:]:
            s = s + x
        cluster_areas.append(s)
    return labels, np.array(counts, np.int64), np.array(cluster_areas,
                                                        np.float64)


def _remap(triangles, vertex_mask):
    """UpdateTriangleIndicesByVertexMask."""
    prefix = np.concatenate([[0], np.cumsum(vertex_mask.astype(np.int64))])
    return prefix[np.asarray(triangles, np.int64)]


def select_faces_by_mask(triangles, v, mask):
    """-> (vertex_mask, triangles_out)."""
    tris = np.asarray(triangles, np.int64).reshape(-1, 3)
    kept = tris[np.asarray(mask, bool)]
    vertex_mask = np.zeros(v, bool)
    vertex_mask[kept.reshape(-1)] = True
    return vertex_mask, _remap(kept, vertex_mask).reshape(-1, 3)


def select_by_index(triangles, v, indices):
    """-> (vertex_mask, tri_mask, triangles_out, n_ignored)."""
    tris = np.asarray(triangles, np.int64).reshape(-1, 3)
    vertex_mask = np.zeros(v, bool)
    ignored = 0
    for i in np.asarray(indices, np.int64).tolist():
        if i < 0 or i >= v:
            ignored += 1
            continue
        vertex_mask[i] = True
    tri_mask = vertex_mask[tris].all(axis=1) if len(tris) else \
        np.zeros(0, bool)
    return (vertex_mask, tri_mask,
            _remap(tris[tri_mask], vertex_mask).reshape(-1, 3), ignored)


def remove_unreferenced_vertices(triangles, v):
    tris = np.asarray(triangles, np.int64).reshape(-1, 3)
    return select_faces_by_mask(tris, v, np.ones(len(tris), bool))
