"""A plain numpy float64 restatement of o3dmi_pointcloud_convex_hull /
o3dmi_pointcloud_hidden_point_removal (include/o3d_mi355x_host.h): a
sequential quickhull with the library's predicate expression and eps, its
initial simplex and tie rules, upstream's flip expression, the same refusals
and the same canonical output. It inserts one point at a time, so wherever the
library's result could depend on its rounds this one does not."""
import numpy as np

OK, INVALID_ARG, CAPACITY, SINGULAR = 0, 1, 3, 5
EPS_ULPS = 256  # kHullEpsUlps / O3DMI_HULL_EPS_ULPS


class HullRefused(Exception):
    def __init__(self, status, why):
        super().__init__(why)
        self.status = status


def eps_of(P):
    """eps = EPS_ULPS * 2^-52 * the largest extent of the bounding box."""
    return (EPS_ULPS * 2.0 ** -52) * float((P.max(axis=0) - P.min(axis=0)).max())


def normal(P, a, b, c):
    """n = (b - a) x (c - a) and |n|, component by component as the kernel."""
    u, v = P[b] - P[a], P[c] - P[a]
    n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2],
                  u[0] * v[1] - u[1] * v[0]])
    return n, float(np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))


def above(P, n, a, idx):
    """(n.x w.x + n.y w.y) + n.z w.z, w = p - a, for the points idx."""
    w = P[idx] - P[a]
    return (n[0] * w[:, 0] + n[1] * w[:, 1]) + n[2] * w[:, 2]


def canonical(tris):
    """Triangles on point indices -> (vertex indices ascending, triangles on
    vertex numbers, each rotated to its lowest first, sorted by rows)."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    verts = np.unique(tris)
    t = np.searchsorted(verts, tris)
    lo = t.argmin(axis=1)
    rows = np.arange(len(t))
    t = np.stack([t[rows, lo], t[rows, (lo + 1) % 3], t[rows, (lo + 2) % 3]],
                 axis=1)
    order = np.lexsort((t[:, 2], t[:, 1], t[:, 0]))
    return verts, t[order]


def _simplex(P, eps):
    x = P[:, 0]
    p0 = int(np.argmax(-x + 0.0))
    p1 = int(np.argmax(x + 0.0))
    e, w = P[p1] - P[p0], P - P[p0]
    cx = w[:, 1] * e[2] - w[:, 2] * e[1]
    cy = w[:, 2] * e[0] - w[:, 0] * e[2]
    cz = w[:, 0] * e[1] - w[:, 1] * e[0]
    p2 = int(np.argmax((cx * cx + cy * cy) + cz * cz))
    n, ln = normal(P, p0, p1, p2)
    p3 = int(np.argmax(np.abs(above(P, n, p0, np.arange(len(P))))))
    h = float(above(P, n, p0, np.array([p3]))[0])
    if not abs(h) > eps * ln:
        raise HullRefused(SINGULAR, "flat")
    a, b, c, d = p0, p1, p2, p3
    if h > 0:
        b, c = c, b
    return [(a, b, c), (a, d, b), (b, d, c), (c, d, a)]


def hull_facets(P):
    """The hull's facets as point-index triples, counter-clockwise from
    outside. P: float64 {m,3}, finite."""
    eps = eps_of(P)
    facets, outside, edge = {}, {}, {}
    next_id = 0

    def add(tri, cand):
        nonlocal next_id
        f = next_id
        next_id += 1
        facets[f] = tri
        for k in range(3):
            edge[(tri[k], tri[(k + 1) % 3])] = f
        n, ln = normal(P, *tri)
        if len(cand):
            out = above(P, n, tri[0], cand) > eps * ln
            outside[f] = cand[out]
            return cand[~out]
        outside[f] = cand
        return cand

    def visible(f, p):
        n, ln = normal(P, *facets[f])
        return above(P, n, facets[f][0], np.array([p]))[0] > eps * ln

    first = _simplex(P, eps)
    rest = np.setdiff1d(np.arange(len(P)), np.array(first[0] + first[1][1:2]))
    for tri in first:
        rest = add(tri, rest)
    work = [f for f in facets if len(outside[f])]
    while work:
        f0 = work.pop()
        if f0 not in facets or not len(outside[f0]):
            continue
        pts = outside[f0]
        n, _ = normal(P, *facets[f0])
        p = int(pts[np.argmax(above(P, n, facets[f0][0], pts))])
        cavity, stack = {f0}, [f0]
        while stack:
            g = stack.pop()
            tri = facets[g]
            for k in range(3):
                h = edge[(tri[(k + 1) % 3], tri[k])]
                if h not in cavity and visible(h, p):
                    cavity.add(h)
                    stack.append(h)
        horizon = []
        for g in sorted(cavity):
            tri = facets[g]
            for k in range(3):
                u, v = tri[k], tri[(k + 1) % 3]
                if edge[(v, u)] not in cavity:
                    horizon.append((u, v))
        orphans = np.concatenate([outside[g] for g in sorted(cavity)])
        orphans = np.sort(orphans[orphans != p])
        for g in cavity:
            for k in range(3):
                del edge[(facets[g][k], facets[g][(k + 1) % 3])]
            del facets[g], outside[g]
        for u, v in horizon:
            before = next_id
            orphans = add((u, v, p), orphans)
            if len(outside[before]):
                work.append(before)
    return np.array([facets[f] for f in sorted(facets)], np.int64)


def _check_points(points, min_n):
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 3 or len(points) < min_n:
        raise HullRefused(INVALID_ARG, "too few points")
    if not np.isfinite(points).all():
        raise HullRefused(INVALID_ARG, "non-finite coordinate")
    return points.astype(np.float64)


def convex_hull(points):
    """-> (point_indices {V}, triangles {T,3} on 0..V-1), both int64."""
    return canonical(hull_facets(_check_points(points, 4)))


def flip(points, camera, radius):
    """Upstream's spherical flip (geometry/PointCloud.cpp:797-804)."""
    v = np.asarray(points, np.float64) - np.asarray(camera, np.float64)
    norm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    with np.errstate(all="ignore"):
        k = 2.0 * (radius - norm)
        return v + (k[:, None] * v) / norm[:, None]


def hidden_point_removal(points, camera, radius):
    """-> (point_indices {V}, triangles {T,3} on 0..V-1), both int64."""
    P = _check_points(points, 3)
    camera = np.asarray(camera, np.float64)
    if not (np.isfinite(camera).all() and np.isfinite(radius) and radius > 0):
        raise HullRefused(INVALID_ARG, "camera or radius")
    f = flip(P, camera, radius)
    if not np.isfinite(f).all():
        raise HullRefused(INVALID_ARG, "flip not finite")
    tris = hull_facets(np.concatenate([f, np.zeros((1, 3))]))
    return canonical(tris[(tris != len(P)).all(axis=1)])


# ---- validity checks shared by the tests ---------------------------------------------
def edges_closed_and_oriented(tris):
    """Every directed edge exactly once and its reverse exactly once."""
    tris = np.asarray(tris, np.int64)
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    fwd = {(int(a), int(b)) for a, b in e}
    return len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd)


def euler(tris):
    tris = np.asarray(tris, np.int64)
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    und = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in e}
    return len(np.unique(tris)) - len(und) + len(tris)
