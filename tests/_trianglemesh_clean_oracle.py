"""CPU restatement (numpy) of the legacy TriangleMesh clean-up calls, the
adjacency list, the four smoothing filters and SimplifyVertexClustering
(geometry/TriangleMesh.cpp:153-440, 680-860, Smoothing.h:29-65,
TriangleMeshSimplification.cpp:72-244) with the orders the device pins:
neighbour lists and cluster members in ascending index, a vertex's triangles
in ascending triangle index, first occurrences kept in input order.

Arithmetic is float64 throughout, as legacy; results are narrowed to the
position dtype at the end. Wherever the order of the additions matters the
sums are sequential: the filters add the k-th neighbour of every vertex in
step k (one elementwise numpy add per step, so every vertex still adds its
own list in list order), the clustering walks plain Python loops.
"""
import math

import numpy as np

SCOPE_ALL, SCOPE_COLOR, SCOPE_NORMAL, SCOPE_VERTEX = 0, 1, 2, 3
AVERAGE, QUADRIC = 0, 1


def expect_eq(got, want, threshold):
    """upstream's ExpectEQ (tests/test_utility/Compare.h:35-57), row by row:
    Eigen's isApprox or an infinity norm within the threshold."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    for a, b in zip(got, want):
        d = a - b
        approx = d @ d <= threshold * threshold * min(a @ a, b @ b)
        assert approx or np.abs(d).max() <= threshold, (a, b)


# ---- representatives ------------------------------------------------------------
def _first_occurrences(keys):
    """rep[i] = the first j with keys[j] == keys[i]; a key of None equals
    nothing (rep = i)."""
    seen, rep = {}, np.empty(len(keys), dtype=np.int64)
    for i, k in enumerate(keys):
        rep[i] = i if k is None else seen.setdefault(k, i)
    return rep


def vertex_keys(positions):
    keys = []
    for row in np.asarray(positions, dtype=np.float64):
        if np.isnan(row).any():
            keys.append(None)
        else:
            keys.append(tuple(float(x) + 0.0 for x in row))  # -0 -> +0
    return keys


def rotate_triangle(t):
    """geometry/TriangleMesh.cpp:744-760."""
    a, b, c = int(t[0]), int(t[1]), int(t[2])
    if a <= b:
        return (a, b, c) if a <= c else (c, a, b)
    return (b, c, a) if b <= c else (c, a, b)


def remove_duplicated_vertices(positions, triangles):
    """-> (vertex mask uint8 {v}, remapped triangles, n kept)."""
    rep = _first_occurrences(vertex_keys(positions))
    first = rep == np.arange(len(rep))
    rank = np.cumsum(first) - first
    new = rank[rep] if len(rep) else rep
    tri = np.asarray(triangles)
    return (first.astype(np.uint8), new[tri.astype(np.int64)].astype(tri.dtype)
            if tri.size else tri.copy(), int(first.sum()))


def remove_duplicated_triangles(triangles):
    """-> (triangle mask uint8 {m}, the kept rows)."""
    tri = np.asarray(triangles)
    rep = _first_occurrences([rotate_triangle(t) for t in tri])
    first = rep == np.arange(len(rep))
    return first.astype(np.uint8), tri[first]


def remove_degenerate_triangles(triangles):
    tri = np.asarray(triangles)
    keep = ((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) &
            (tri[:, 2] != tri[:, 0])) if tri.size else np.zeros(0, bool)
    return keep.astype(np.uint8), tri[keep]


# ---- adjacency ------------------------------------------------------------------
def adjacency_sets(triangles, v):
    """Legacy ComputeAdjacencyList, the six inserts per triangle."""
    adj = [set() for _ in range(v)]
    for t in np.asarray(triangles):
        a, b, c = int(t[0]), int(t[1]), int(t[2])
        adj[a].add(b)
        adj[a].add(c)
        adj[b].add(a)
        adj[b].add(c)
        adj[c].add(a)
        adj[c].add(b)
    return adj


def adjacency_csr(triangles, v):
    """-> (row_splits int64 {v+1}, neighbours int64), lists ascending."""
    lists = [sorted(s) for s in adjacency_sets(triangles, v)]
    splits = np.zeros(v + 1, dtype=np.int64)
    splits[1:] = np.cumsum([len(x) for x in lists])
    flat = [x for lst in lists for x in lst]
    return splits, np.asarray(flat, dtype=np.int64)


# ---- filters ----------------------------------------------------------------------
def _steps(splits, nbrs):
    """For k = 0, 1, ...: (the vertices with more than k neighbours, their
    k-th neighbour)."""
    deg = np.diff(splits)
    for k in range(int(deg.max()) if len(deg) else 0):
        who = np.nonzero(deg > k)[0]
        yield who, nbrs[splits[who] + k]


def _plain_pass(kind, splits, nbrs, attrs, factor):
    nb = np.diff(splits).astype(np.float64)[:, None]
    out = []
    for prev in attrs:
        total = np.zeros_like(prev)
        for who, other in _steps(splits, nbrs):
            total[who] = total[who] + prev[other]
        if kind == "sharpen":
            out.append(prev + factor * (prev * nb - total))
        else:
            out.append((prev + total) / (1.0 + nb))
    return out


def _laplacian_pass(splits, nbrs, ref, attrs, factor):
    weight_sum = np.zeros(len(ref))
    sums = [np.zeros_like(a) for a in attrs]
    for who, other in _steps(splits, nbrs):
        d = ref[who] - ref[other]
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) +
                       d[:, 2] * d[:, 2])
        w = 1.0 / (dist + 1e-12)
        weight_sum[who] = weight_sum[who] + w
        for s, prev in zip(sums, attrs):
            s[who] = s[who] + w[:, None] * prev[other]
    ok = weight_sum > 0.0
    out = []
    for s, prev in zip(sums, attrs):
        nxt = prev.copy()
        nxt[ok] = prev[ok] + factor * (s[ok] / weight_sum[ok][:, None] -
                                       prev[ok])
        out.append(nxt)
    return out


def run_filter(kind, positions, normals, colors, triangles, iterations,
               factors, scope):
    """kind: "sharpen" (factors = [strength]), "simple" ([]), "laplacian"
    ([lambda]) or "taubin" ([lambda, mu]). -> (positions, normals, colors)
    in the input dtypes; an attribute outside the scope (or None) comes back
    as it went in."""
    dtype = positions.dtype
    given = [positions, normals, colors]
    wanted = [scope in (SCOPE_ALL, SCOPE_VERTEX),
              scope in (SCOPE_ALL, SCOPE_NORMAL) and normals is not None,
              scope in (SCOPE_ALL, SCOPE_COLOR) and colors is not None]
    result = [None if a is None else a.copy() for a in given]
    if iterations <= 0 or not any(wanted):
        return tuple(result)
    splits, nbrs = adjacency_csr(triangles, len(positions))
    slots = [i for i in range(3) if wanted[i]]
    attrs = [given[i].astype(np.float64) for i in slots]
    fixed = None if wanted[0] else positions.astype(np.float64)
    if kind in ("sharpen", "simple"):
        factor = factors[0] if factors else 0.0
        for _ in range(iterations):
            attrs = _plain_pass(kind, splits, nbrs, attrs, factor)
    else:
        per_iter = [factors[0]] if kind == "laplacian" else list(factors)
        for _ in range(iterations):
            for factor in per_iter:
                ref = attrs[0] if fixed is None else fixed
                attrs = _laplacian_pass(splits, nbrs, ref, attrs, factor)
    for i, a in zip(slots, attrs):
        result[i] = a.astype(dtype)
    return tuple(result)


# ---- vertex clustering ------------------------------------------------------------
def voxel_indices(positions, voxel_size):
    p = np.asarray(positions, dtype=np.float64)
    min_bound = p.min(axis=0) - voxel_size * 0.5
    return np.floor((p - min_bound) / voxel_size).astype(np.int32)


def voxel_size_ok(positions, voxel_size):
    """Upstream's two refusals."""
    if not voxel_size > 0.0:
        return False
    p = np.asarray(positions, dtype=np.float64)
    lo = p.min(axis=0) - voxel_size * 0.5
    hi = p.max(axis=0) + voxel_size * 0.5
    return not voxel_size * float(2 ** 31 - 1) < float((hi - lo).max())


def triangle_plane(p0, p1, p2):
    """ComputeTrianglePlane, geometry/TriangleMesh.cpp:1248-1262 (Python
    floats)."""
    e0 = [p1[k] - p0[k] for k in range(3)]
    e1 = [p2[k] - p0[k] for k in range(3)]
    abc = [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2],
           e0[0] * e1[1] - e0[1] * e1[0]]
    norm = math.sqrt((abc[0] * abc[0] + abc[1] * abc[1]) + abc[2] * abc[2])
    if norm == 0:
        return [0.0, 0.0, 0.0, 0.0]
    n = [x / norm for x in abc]
    return n + [-((n[0] * p0[0] + n[1] * p0[1]) + n[2] * p0[2])]


def triangle_area(p0, p1, p2):
    """Legacy ComputeTriangleArea: 0.5 |(p0 - p1) x (p0 - p2)|."""
    x = [p0[k] - p1[k] for k in range(3)]
    y = [p0[k] - p2[k] for k in range(3)]
    c = [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2],
         x[0] * y[1] - x[1] * y[0]]
    return 0.5 * math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])


def quadric_minimum(q):
    """q: A row-major (9), then b (3) -> the minimiser, or None when
    |det| > 1e-4 fails."""
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = q[:9]
    m00 = a11 * a22 - a12 * a21
    m01 = a10 * a22 - a12 * a20
    m02 = a10 * a21 - a11 * a20
    det = a00 * m00 - a01 * m01 + a02 * m02
    if not abs(det) > 1e-4:
        return None
    c = [[m00, -m01, m02],
         [-(a01 * a22 - a02 * a21), a00 * a22 - a02 * a20,
          -(a00 * a21 - a01 * a20)],
         [a01 * a12 - a02 * a11, -(a00 * a12 - a02 * a10),
          a00 * a11 - a01 * a10]]
    b = q[9:12]
    return [-((c[i][0] * b[0] + c[i][1] * b[1]) + c[i][2] * b[2]) / det
            for i in range(3)]


def simplify_vertex_clustering(positions, normals, colors, triangles,
                               voxel_size, contraction):
    """-> dict(positions, normals, colors, triangles, new_index)."""
    dtype = positions.dtype
    p = positions.astype(np.float64)
    v = len(p)
    vox = voxel_indices(p, voxel_size)
    new_of_voxel, new_index, members = {}, np.empty(v, dtype=np.int64), []
    for i in range(v):
        key = tuple(int(x) for x in vox[i])
        if key not in new_of_voxel:
            new_of_voxel[key] = len(members)
            members.append([])
        new_index[i] = new_of_voxel[key]
        members[new_index[i]].append(i)  # ascending old index
    tri = np.asarray(triangles).astype(np.int64)

    def average(values):
        rows = values.astype(np.float64).tolist()
        out = np.empty((len(members), 3))
        for c, mem in enumerate(members):
            s = [0.0, 0.0, 0.0]
            for i in mem:
                s = [s[k] + rows[i][k] for k in range(3)]
            out[c] = [s[k] / float(len(mem)) for k in range(3)]
        return out

    out_p = average(p)
    if contraction == QUADRIC and len(tri):
        rows = p.tolist()
        of_vertex = [[] for _ in range(v)]
        for t, (a, b, c) in enumerate(tri.tolist()):
            for u in (a, b, c):
                if not of_vertex[u] or of_vertex[u][-1] != t:
                    of_vertex[u].append(t)
        plane = [triangle_plane(rows[a], rows[b], rows[c])
                 for a, b, c in tri.tolist()]
        area = [triangle_area(rows[a], rows[b], rows[c])
                for a, b, c in tri.tolist()]
        for c, mem in enumerate(members):
            q = [0.0] * 12
            for i in mem:
                for t in of_vertex[i]:
                    n, d, w = plane[t][:3], plane[t][3], area[t]
                    for r in range(3):
                        wn = w * n[r]
                        for s in range(3):
                            q[3 * r + s] += wn * n[s]
                    wd = w * d
                    for r in range(3):
                        q[9 + r] += wd * n[r]
            x = quadric_minimum(q)
            if x is not None:
                out_p[c] = x
    kept, seen = [], set()
    for a, b, c in tri.tolist():
        v0, v1, v2 = int(new_index[a]), int(new_index[b]), int(new_index[c])
        if v0 == v1 or v0 == v2 or v1 == v2:
            continue
        if v1 < v0 and v1 < v2:
            v0, v1, v2 = v1, v2, v0
        elif v2 < v0 and v2 < v1:
            v0, v1, v2 = v2, v0, v1
        if (v0, v1, v2) not in seen:
            seen.add((v0, v1, v2))
            kept.append((v0, v1, v2))
    return dict(
        positions=out_p.astype(dtype),
        normals=None if normals is None else average(normals).astype(dtype),
        colors=None if colors is None else average(colors).astype(dtype),
        triangles=np.asarray(kept, dtype=np.asarray(triangles).dtype)
        .reshape(-1, 3),
        new_index=new_index)
