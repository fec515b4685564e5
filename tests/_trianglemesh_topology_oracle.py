"""CPU restatement of the mesh topology and intersection queries, numpy and
plain Python: (1) a literal transcription of the legacy loops
(geometry/TriangleMesh.cpp:1016-1135, 1212-1246, 1272-1457 and
IntersectionTest::AABBAABB / TriangleTriangle3d with Moeller's no-division
test in Python floats, which are IEEE doubles without contraction), (2) the
definitions the C ABI states, as independent brute-force code, (3) an exact
triangle-triangle test in fractions, and (4) small mesh makers."""
import math
from collections import deque
from fractions import Fraction

import numpy as np


# ---- (1) upstream's loops, literally ------------------------------------------------
def ordered_edge(a, b):
    return (min(a, b), max(a, b))


def euler_poincare_characteristic(n_vertices, triangles):
    edges = set()
    for t in triangles:
        edges.add(ordered_edge(t[0], t[1]))
        edges.add(ordered_edge(t[0], t[2]))
        edges.add(ordered_edge(t[1], t[2]))
    return n_vertices + len(triangles) - len(edges)


def edge_to_triangles(triangles):
    edges = {}
    for tidx, t in enumerate(triangles):
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            edges.setdefault(ordered_edge(a, b), []).append(tidx)
    return edges


def is_edge_manifold(triangles, allow_boundary_edges=True):
    for tris in edge_to_triangles(triangles).values():
        if allow_boundary_edges and (len(tris) < 1 or len(tris) > 2):
            return False
        if not allow_boundary_edges and len(tris) != 2:
            return False
    return True


def get_non_manifold_vertices(n_vertices, triangles):
    """The legacy loop; the empty edge map, which upstream dereferences, is
    skipped."""
    vert_to_triangles = [set() for _ in range(n_vertices)]
    for tidx, t in enumerate(triangles):
        for k in range(3):
            vert_to_triangles[t[k]].add(tidx)
    out = []
    for vidx in range(n_vertices):
        tris = vert_to_triangles[vidx]
        if not tris:
            continue
        edges = {}
        for tidx in tris:
            t = triangles[tidx]
            if t[0] != vidx and t[1] != vidx:
                edges.setdefault(t[0], set()).add(t[1])
                edges.setdefault(t[1], set()).add(t[0])
            elif t[0] != vidx and t[2] != vidx:
                edges.setdefault(t[0], set()).add(t[2])
                edges.setdefault(t[2], set()).add(t[0])
            elif t[1] != vidx and t[2] != vidx:
                edges.setdefault(t[1], set()).add(t[2])
                edges.setdefault(t[2], set()).add(t[1])
        if not edges:
            continue  # upstream: edges.begin() of an empty map
        first = next(iter(edges))
        queue, visited = deque([first]), {first}
        while queue:
            vert = queue.popleft()
            for nb in edges[vert]:
                if nb not in visited:
                    visited.add(nb)
                    queue.append(nb)
        if len(visited) != len(edges):
            out.append(vidx)
    return out


def orient_triangles(triangles):
    """OrientTriangleHelper with the next unvisited triangle chosen in sorted
    order (upstream: *unordered_set.begin()) and adjacent triangles queued in
    ascending order. -> (orientable, triangles as upstream leaves them)."""
    tris = [list(map(int, t)) for t in triangles]
    edge_to_orientation = {}
    unvisited = set(range(len(tris)))
    adjacent = {}
    queue = deque()
    for tidx, t in enumerate(tris):
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            adjacent.setdefault(ordered_edge(a, b), set()).add(tidx)

    def verify_and_add(v0, v1):
        key = ordered_edge(v0, v1)
        if key in edge_to_orientation:
            if edge_to_orientation[key][0] == v0:
                return False
        else:
            edge_to_orientation[key] = (v0, v1)
        return True

    while unvisited:
        if not queue:
            tidx = min(unvisited)
        else:
            tidx = queue.popleft()
        if tidx in unvisited:
            unvisited.remove(tidx)
        else:
            continue
        v0, v1, v2 = tris[tidx]
        key01, key12, key20 = (ordered_edge(v0, v1), ordered_edge(v1, v2),
                               ordered_edge(v2, v0))
        e01 = key01 in edge_to_orientation
        e12 = key12 in edge_to_orientation
        e20 = key20 in edge_to_orientation
        if not (e01 or e12 or e20):
            edge_to_orientation[key01] = (v0, v1)
            edge_to_orientation[key12] = (v1, v2)
            edge_to_orientation[key20] = (v2, v0)
        else:
            t = tris[tidx]
            if e01 and edge_to_orientation[key01][0] == v0:
                v0, v1 = v1, v0
                t[0], t[1] = t[1], t[0]
            elif e12 and edge_to_orientation[key12][0] == v1:
                v1, v2 = v2, v1
                t[1], t[2] = t[2], t[1]
            elif e20 and edge_to_orientation[key20][0] == v2:
                v2, v0 = v0, v2
                t[2], t[0] = t[0], t[2]
            if not verify_and_add(v0, v1):
                return False, tris
            if not verify_and_add(v1, v2):
                return False, tris
            if not verify_and_add(v2, v0):
                return False, tris
        for key in (key01, key12, key20):
            for nb in sorted(adjacent[key]):
                queue.append(nb)
    return True, tris


def aabb_aabb(min0, max0, min1, max1):
    for k in range(3):
        if max0[k] < min1[k] or min0[k] > max1[k]:
            return False
    return True


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2],
            a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _edge_edge(v0, ax, ay, u0, u1, i0, i1):
    bx = u0[i0] - u1[i0]
    by = u0[i1] - u1[i1]
    cx = v0[i0] - u0[i0]
    cy = v0[i1] - u0[i1]
    f = ay * bx - ax * by
    d = by * cx - bx * cy
    if (f > 0 and d >= 0 and d <= f) or (f < 0 and d <= 0 and d >= f):
        e = ax * cy - ay * cx
        if f > 0:
            if e >= 0 and e <= f:
                return True
        else:
            if e <= 0 and e >= f:
                return True
    return False


def _edge_against_tri(v0, v1, u, i0, i1):
    ax = v1[i0] - v0[i0]
    ay = v1[i1] - v0[i1]
    return (_edge_edge(v0, ax, ay, u[0], u[1], i0, i1) or
            _edge_edge(v0, ax, ay, u[1], u[2], i0, i1) or
            _edge_edge(v0, ax, ay, u[2], u[0], i0, i1))


def _point_in_tri(p, u, i0, i1):
    ds = []
    for a_, b_ in ((u[0], u[1]), (u[1], u[2]), (u[2], u[0])):
        a = b_[i1] - a_[i1]
        b = -(b_[i0] - a_[i0])
        c = -a * a_[i0] - b * a_[i1]
        ds.append(a * p[i0] + b * p[i1] + c)
    return ds[0] * ds[1] > 0.0 and ds[0] * ds[2] > 0.0


def coplanar_tri_tri(n, v, u):
    a = [abs(n[0]), abs(n[1]), abs(n[2])]
    if a[0] > a[1]:
        i0, i1 = (1, 2) if a[0] > a[2] else (0, 1)
    else:
        i0, i1 = (0, 1) if a[2] > a[1] else (0, 2)
    if _edge_against_tri(v[0], v[1], u, i0, i1):
        return True
    if _edge_against_tri(v[1], v[2], u, i0, i1):
        return True
    if _edge_against_tri(v[2], v[0], u, i0, i1):
        return True
    return _point_in_tri(v[0], u, i0, i1) or _point_in_tri(u[0], v, i0, i1)


def _interval(vv0, vv1, vv2, d0, d1, d2, d0d1, d0d2):
    """-> (a, b, c, x0, x1) or None for coplanar triangles."""
    if d0d1 > 0.0:
        return vv2, (vv0 - vv2) * d2, (vv1 - vv2) * d2, d2 - d0, d2 - d1
    if d0d2 > 0.0:
        return vv1, (vv0 - vv1) * d1, (vv2 - vv1) * d1, d1 - d0, d1 - d2
    if d1 * d2 > 0.0 or d0 != 0.0:
        return vv0, (vv1 - vv0) * d0, (vv2 - vv0) * d0, d0 - d1, d0 - d2
    if d1 != 0.0:
        return vv1, (vv0 - vv1) * d1, (vv2 - vv1) * d1, d1 - d0, d1 - d2
    if d2 != 0.0:
        return vv2, (vv0 - vv2) * d2, (vv1 - vv2) * d2, d2 - d0, d2 - d1
    return None


EPSILON = 0.000001


def plane_distances(v, u):
    """The three distances of u's vertices to v's plane, before the snap."""
    n1 = _cross(_sub(v[1], v[0]), _sub(v[2], v[0]))
    d1 = -_dot(n1, v[0])
    return n1, [_dot(n1, u[k]) + d1 for k in range(3)]


def no_div_tri_tri_isect(v, u):
    n1, du = plane_distances(v, u)
    du = [0.0 if abs(x) < EPSILON else x for x in du]
    du0du1 = du[0] * du[1]
    du0du2 = du[0] * du[2]
    if du0du1 > 0.0 and du0du2 > 0.0:
        return False
    n2, dv = plane_distances(u, v)
    dv = [0.0 if abs(x) < EPSILON else x for x in dv]
    dv0dv1 = dv[0] * dv[1]
    dv0dv2 = dv[0] * dv[2]
    if dv0dv1 > 0.0 and dv0dv2 > 0.0:
        return False
    d = _cross(n1, n2)
    mx, index = abs(d[0]), 0
    bb, cc = abs(d[1]), abs(d[2])
    if bb > mx:
        mx, index = bb, 1
    if cc > mx:
        mx, index = cc, 2
    iv = _interval(v[0][index], v[1][index], v[2][index], dv[0], dv[1], dv[2],
                   dv0dv1, dv0dv2)
    if iv is None:
        return coplanar_tri_tri(n1, v, u)
    a, b, c, x0, x1 = iv
    iu = _interval(u[0][index], u[1][index], u[2][index], du[0], du[1], du[2],
                   du0du1, du0du2)
    if iu is None:
        return coplanar_tri_tri(n1, v, u)
    d_, e, f, y0, y1 = iu
    xx = x0 * x1
    yy = y0 * y1
    xxyy = xx * yy
    tmp = a * xxyy
    s = sorted((tmp + b * x1 * yy, tmp + c * x0 * yy))
    tmp = d_ * xxyy
    t = sorted((tmp + e * xx * y1, tmp + f * xx * y0))
    return not (s[1] < t[0] or t[1] < s[0])


def normalise_pair(p, q):
    """TriangleTriangle3d's mu / sigma normalisation of six points."""
    pts = [list(map(float, x)) for x in list(p) + list(q)]
    out = [[0.0] * 3 for _ in range(6)]
    for k in range(3):
        mu = (((((pts[0][k] + pts[1][k]) + pts[2][k]) + pts[3][k]) +
               pts[4][k]) + pts[5][k]) / 6
        dev = [x[k] - mu for x in pts]
        sq = dev[0] * dev[0] + dev[1] * dev[1]
        for j in range(2, 6):
            sq = sq + dev[j] * dev[j]
        sigma = math.sqrt(sq / 5) + 1e-12
        for j in range(6):
            out[j][k] = dev[j] / sigma
    return out[:3], out[3:]


def triangle_triangle_3d(p, q):
    pn, qn = normalise_pair(p, q)
    return no_div_tri_tri_isect(pn, qn)


def tri_box(t):
    return ([min(t[0][k], t[1][k], t[2][k]) for k in range(3)],
            [max(t[0][k], t[1][k], t[2][k]) for k in range(3)])


def pair_counts(p, q):
    """The per-pair function: boxes overlap and hit."""
    return aabb_aabb(*tri_box(p), *tri_box(q)) and triangle_triangle_3d(p, q)


def shares_vertex(a, b):
    return any(x == y for x in a for y in b)


def get_self_intersecting_triangles(positions, triangles):
    """The legacy all-pairs loop -> (pairs in ascending (i, j), the number of
    TriangleTriangle3d calls)."""
    pos = np.asarray(positions, np.float64).tolist()
    tris = np.asarray(triangles).tolist()
    out, tested = [], 0
    for i in range(len(tris)):
        p = [pos[x] for x in tris[i]]
        pb = tri_box(p)
        for j in range(i + 1, len(tris)):
            if shares_vertex(tris[i], tris[j]):
                continue
            q = [pos[x] for x in tris[j]]
            if aabb_aabb(*pb, *tri_box(q)):
                tested += 1
                if triangle_triangle_3d(p, q):
                    out.append((i, j))
    return out, tested


def box_candidates(positions, triangles, other_positions=None,
                   other_triangles=None):
    """The (i, j) whose float64 boxes overlap (closed), by numpy, in
    ascending (i, j); one mesh: i < j only."""
    pos = np.asarray(positions, np.float64)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    self_query = other_triangles is None
    opos = pos if self_query else np.asarray(other_positions, np.float64)
    otri = tri if self_query else np.asarray(other_triangles,
                                             np.int64).reshape(-1, 3)
    lo, hi = pos[tri].min(1), pos[tri].max(1)
    olo, ohi = opos[otri].min(1), opos[otri].max(1)
    out = []
    for i in range(len(tri)):
        ok = ~((hi[i] < olo) | (lo[i] > ohi)).any(1)
        if self_query:
            ok[:i + 1] = False
        out.extend((i, int(j)) for j in np.nonzero(ok)[0])
    return out


def self_intersections(positions, triangles):
    """get_self_intersecting_triangles with the box test done first in numpy
    (the same pairs, the same count)."""
    pos = np.asarray(positions, np.float64).tolist()
    tris = np.asarray(triangles).tolist()
    out, tested = [], 0
    for i, j in box_candidates(positions, triangles):
        if shares_vertex(tris[i], tris[j]):
            continue
        tested += 1
        if triangle_triangle_3d([pos[x] for x in tris[i]],
                                [pos[x] for x in tris[j]]):
            out.append((i, j))
    return out, tested


def bounds(positions):
    p = np.asarray(positions, np.float64).reshape(-1, 3)
    return p.min(0).tolist(), p.max(0).tolist()


def is_intersecting(positions, triangles, other_positions, other_triangles,
                    per_pair_box=True):
    """Legacy IsIntersecting; per_pair_box=False is upstream's own loop, True
    the C ABI's stated difference."""
    if len(triangles) == 0 or len(other_triangles) == 0:
        return False
    if not aabb_aabb(*bounds(positions), *bounds(other_positions)):
        return False
    pos = np.asarray(positions, np.float64).tolist()
    opos = np.asarray(other_positions, np.float64).tolist()
    for a in np.asarray(triangles).tolist():
        p = [pos[x] for x in a]
        for b in np.asarray(other_triangles).tolist():
            q = [opos[x] for x in b]
            if per_pair_box and not aabb_aabb(*tri_box(p), *tri_box(q)):
                continue
            if triangle_triangle_3d(p, q):
                return True
    return False


def volume_terms(positions, triangles):
    """p0 . (p1 x p2) / 6 per triangle, in Python floats."""
    pos = np.asarray(positions, np.float64).tolist()
    out = []
    for t in np.asarray(triangles).tolist():
        p0, p1, p2 = (pos[x] for x in t)
        c = _cross(p1, p2)
        out.append(((p0[0] * c[0] + p0[1] * c[1]) + p0[2] * c[2]) / 6.0)
    return out


def is_watertight(positions, triangles):
    n = len(positions)
    tris = np.asarray(triangles).tolist()
    return (is_edge_manifold(tris, False) and
            not wedge_non_manifold_vertices(n, tris) and
            not self_intersections(positions, triangles)[0])


def get_volume(positions, triangles):
    """Upstream's left-to-right sum of the terms, absolute."""
    total = 0.0
    for x in volume_terms(positions, triangles):
        total += x
    return abs(total)


# ---- (2) the stated definitions, brute force ---------------------------------------
def _components(nodes, edges):
    parent = {x: x for x in nodes}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return {x: find(x) for x in nodes}


def wedge_non_manifold_vertices(n_vertices, triangles):
    """x is non-manifold iff the link edges of its wedges (triangles that name
    x exactly once) form more than one connected component."""
    links = [[] for _ in range(n_vertices)]
    for t in triangles:
        t = list(map(int, t))
        for x in set(t):
            if t.count(x) == 1:
                links[x].append(tuple(y for y in t if y != x))
    out = []
    for x, edges in enumerate(links):
        if not edges:
            continue
        nodes = {y for e in edges for y in e}
        if len(set(_components(nodes, edges).values())) > 1:
            out.append(x)
    return out


def orientation_constraints(triangles):
    """-> (constraints [(t, u, parity)], whether an edge has multiplicity > 2).
    parity 1: t and u run the edge the same way, exactly one must flip."""
    slots = {}
    for tidx, t in enumerate(triangles):
        for k in range(3):
            a, b = int(t[k]), int(t[(k + 1) % 3])
            if a != b:
                slots.setdefault(ordered_edge(a, b), []).append((tidx, a < b))
    cons, fan = [], False
    for s in slots.values():
        if len(s) > 2:
            fan = True
        elif len(s) == 2 and s[0][0] != s[1][0]:
            cons.append((s[0][0], s[1][0], int(s[0][1] == s[1][1])))
    return cons, fan


def canonical_orientation(triangles):
    """-> (orientable, triangles_out): flips propagated breadth first from the
    lowest triangle of every component, then every constraint checked."""
    tris = [list(map(int, t)) for t in triangles]
    cons, fan = orientation_constraints(tris)
    nbrs = [[] for _ in tris]
    for t, u, p in cons:
        nbrs[t].append((u, p))
        nbrs[u].append((t, p))
    flip = [None] * len(tris)
    for seed in range(len(tris)):
        if flip[seed] is not None:
            continue
        flip[seed] = 0
        queue = deque([seed])
        while queue:
            t = queue.popleft()
            for u, p in nbrs[t]:
                if flip[u] is None:
                    flip[u] = flip[t] ^ p
                    queue.append(u)
    ok = not fan and all(flip[t] ^ flip[u] == p for t, u, p in cons)
    if not ok:
        return False, tris
    return True, [[t[0], t[2], t[1]] if f else t for t, f in zip(tris, flip)]


def rotate_min_first(t):
    k = min(range(3), key=lambda i: (t[i], i))
    return (t[k], t[(k + 1) % 3], t[(k + 2) % 3])


# ---- (3) exact intersection in fractions -----------------------------------------------
def _frac(t):
    return [[Fraction(float(x)) for x in p] for p in t]


def _segment_pierces(a, b, tri):
    """Whether the segment (a, b) meets the triangle, exactly (general
    position: the segment is not parallel to the plane)."""
    n = _cross(_sub(tri[1], tri[0]), _sub(tri[2], tri[0]))
    da, db = _dot(n, _sub(a, tri[0])), _dot(n, _sub(b, tri[0]))
    if da == db or (da > 0) == (db > 0) and da != 0 and db != 0:
        return False
    s = da / (da - db)
    x = [a[k] + s * (b[k] - a[k]) for k in range(3)]
    signs = []
    for k in range(3):
        e = _sub(tri[(k + 1) % 3], tri[k])
        signs.append(_dot(n, _cross(e, _sub(x, tri[k]))))
    return all(v >= 0 for v in signs) or all(v <= 0 for v in signs)


def exact_intersects(p, q):
    """Two triangles in general position meet iff an edge of one pierces the
    other."""
    p, q = _frac(p), _frac(q)
    for k in range(3):
        if _segment_pierces(p[k], p[(k + 1) % 3], q):
            return True
        if _segment_pierces(q[k], q[(k + 1) % 3], p):
            return True
    return False


def min_plane_distance(p, q):
    """The smallest of the six normalised plane distances, before the snap."""
    pn, qn = normalise_pair(p, q)
    return min(abs(x) for x in plane_distances(pn, qn)[1] +
               plane_distances(qn, pn)[1])


# ---- (4) mesh makers ---------------------------------------------------------------------
def make_sphere(radius=1.0, resolution=20):
    """A UV sphere in upstream's layout: two poles, resolution - 1 rings of
    2 resolution vertices, outward winding."""
    r2 = 2 * resolution
    verts = [[0.0, 0.0, radius], [0.0, 0.0, -radius]]
    step = math.pi / resolution
    for i in range(1, resolution):
        alpha = step * i
        for j in range(r2):
            theta = step * j
            verts.append([math.sin(alpha) * math.cos(theta) * radius,
                          math.sin(alpha) * math.sin(theta) * radius,
                          math.cos(alpha) * radius])
    tris = []
    last = 2 + r2 * (resolution - 2)
    for j in range(r2):
        j1 = (j + 1) % r2
        tris.append([0, 2 + j, 2 + j1])
        tris.append([1, last + j1, last + j])
    for i in range(1, resolution - 1):
        b1 = 2 + r2 * (i - 1)
        b2 = b1 + r2
        for j in range(r2):
            j1 = (j + 1) % r2
            tris.append([b2 + j, b1 + j1, b1 + j])
            tris.append([b2 + j, b2 + j1, b1 + j1])
    return np.array(verts), np.array(tris, np.int32)


def make_torus(torus_radius=1.0, tube_radius=0.5, radial=30, tubular=20):
    verts = []
    for i in range(radial):
        u = 2 * math.pi * i / radial
        for j in range(tubular):
            w = 2 * math.pi * j / tubular
            r = torus_radius + tube_radius * math.cos(w)
            verts.append([r * math.cos(u), r * math.sin(u),
                          tube_radius * math.sin(w)])
    tris = []
    for i in range(radial):
        i1 = (i + 1) % radial
        for j in range(tubular):
            j1 = (j + 1) % tubular
            a, b = i * tubular + j, i1 * tubular + j
            c, d = i1 * tubular + j1, i * tubular + j1
            tris.append([a, b, c])
            tris.append([a, c, d])
    return np.array(verts), np.array(tris, np.int32)


def make_cone(n, radius=1.0, height=2.0, closed=True):
    """Apex 0 with a fan of n triangles over a ring 1..n; closed: a base fan
    around vertex n + 1."""
    verts = [[0.0, 0.0, height]]
    for j in range(n):
        a = 2 * math.pi * j / n
        verts.append([radius * math.cos(a), radius * math.sin(a), 0.0])
    tris = [[0, 1 + j, 1 + (j + 1) % n] for j in range(n)]
    if closed:
        verts.append([0.0, 0.0, 0.0])
        tris += [[n + 1, 1 + (j + 1) % n, 1 + j] for j in range(n)]
    return np.array(verts), np.array(tris, np.int32)


def make_mobius(n, width=0.4):
    """A Moebius strip of n quads: two rims of n vertices, the last quad joins
    the rims crosswise."""
    verts = []
    for side in (-1.0, 1.0):
        for j in range(n):
            u = 2 * math.pi * j / n
            s = side * width
            r = 1.0 + s * math.cos(u / 2)
            verts.append([r * math.cos(u), r * math.sin(u),
                          s * math.sin(u / 2)])
    tris = []
    for j in range(n):
        a, b = j, n + j
        if j + 1 < n:
            c, d = j + 1, n + j + 1
        else:
            c, d = n, 0  # the half twist
        tris.append([a, c, b])
        tris.append([b, c, d])
    return np.array(verts), np.array(tris, np.int32)


def make_grid(nx, ny, spacing=1.0):
    """A flat grid of nx x ny cells in z = 0, two triangles a cell."""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    verts = np.stack([xs.ravel() * spacing, ys.ravel() * spacing,
                      np.zeros(xs.size)], 1).astype(np.float64)
    cx, cy = np.meshgrid(np.arange(nx), np.arange(ny))
    a = (cy * (nx + 1) + cx).ravel()
    b, c, d = a + 1, a + nx + 2, a + nx + 1
    tris = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)],
                    1).reshape(-1, 3)
    return verts, tris.astype(np.int32)
