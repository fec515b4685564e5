"""numpy restatement of TriangleMesh sampling, the closest-point queries and
TriangleMesh::ComputeMetrics as include/o3d_mi355x_host.h pins them:

  draw      h_k = SplitMix64(seed + GOLDEN * (3 j + k + 1)) mod 2^64;
            u = (h_0 >> 11) 2^-53, r1 = (h_1 >> 40) 2^-24, r2 = (h_2 >> 40) 2^-24
  triangle  the prefix tree over the areas (groups of RUN, prefixes added in
            index order, a level of group totals on top until one group is
            left) and its descent
  point     upstream's mix_3x3 with float weights, no contraction
  d2(q, t)  max(e2, b2): upstream's closestPointTriangle in np.float32, every
            dot product (x x + y y) + z z, clamped by the distance to the
            triangle's own box; a NaN e2 stays NaN
  query     an exhaustive loop over all (q, t): the minimum d2, the lowest
            index among equals, NaN never wins

It never builds a tree.
"""
import json
import os

import numpy as np

import _pointcloud_metrics_oracle as pm
import _trianglemesh_oracle as tm

RUN = 512
MASK = (1 << 64) - 1
GOLDEN_RATIO = 0x9E3779B97F4A7C15
NO_TRIANGLE = 0xFFFFFFFF
F32 = np.float32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "mesh_distance_vectors.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- the draw ----------------------------------------------------------------
def splitmix64(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def draw(seed, j):
    """-> (u float64, r1 float32, r2 float32), all in [0, 1)."""
    c = 3 * j
    h = [splitmix64(seed + GOLDEN_RATIO * (c + k + 1)) for k in range(3)]
    u = np.float64(h[0] >> 11) * np.float64(2.0 ** -53)
    r1 = F32(h[1] >> 40) * F32(2.0 ** -24)
    r2 = F32(h[2] >> 40) * F32(2.0 ** -24)
    return u, r1, r2


# ---- the triangle choice -------------------------------------------------------
def _group_prefix(values):
    v = np.asarray(values, np.float64)
    out = np.empty_like(v)
    for s in range(0, len(v), RUN):
        out[s:s + RUN] = np.cumsum(v[s:s + RUN])  # left to right
    return out


def prefix_levels(areas):
    """-> [(values, prefix)] from level 0 up; the last level is one group."""
    values = np.asarray(areas).astype(np.float64)
    assert len(values) >= 1
    levels = []
    while True:
        prefix = _group_prefix(values)
        levels.append((values, prefix))
        if len(values) <= RUN:
            return levels
        last = np.minimum(np.arange(RUN, len(values) + RUN, RUN),
                          len(values)) - 1
        values = prefix[last]


def total_area(levels):
    return levels[-1][1][-1]


def descend(levels, u):
    """The triangle u in [0, 1) picks."""
    x = np.float64(u) * total_area(levels)
    group = 0
    for values, prefix in reversed(levels):
        base = group * RUN
        p = prefix[base:base + RUN]
        i = int(np.searchsorted(p, x, side="right"))  # first i with x < p[i]
        if i == len(p):
            own = values[base:base + RUN]
            i = int(np.flatnonzero(own > 0)[-1])
        if i > 0:
            x = x - p[i - 1]
        group = base + i
    return group


# ---- the point -------------------------------------------------------------------
def _mix(a, b, c, w0, w1, w2):
    return (w0[:, None] * a + w1[:, None] * b) + w2[:, None] * c


def colors_as_float(colors):
    colors = np.asarray(colors)
    if colors.dtype == np.uint8:
        return colors.astype(F32) / F32(255)
    if colors.dtype == np.uint16:
        return colors.astype(F32) / F32(65535)
    return colors.astype(F32)


def sample(positions, triangles, n, seed, vertex_normals=None,
           triangle_normals=None, vertex_colors=None):
    """-> dict(triangles int32 {n}, points, normals / colors when given)."""
    positions = np.asarray(positions)
    tri = np.asarray(triangles, np.int64)
    with np.errstate(all="ignore"):
        areas = tm.triangle_areas(positions, tri)
    levels = prefix_levels(areas)
    draws = [draw(seed, j) for j in range(n)]
    t = np.array([descend(levels, d[0]) for d in draws], np.int64)
    r1 = np.array([d[1] for d in draws], F32)
    r2 = np.array([d[2] for d in draws], F32)
    s1 = np.sqrt(r1)
    w0, w1, w2 = F32(1) - s1, s1 * (F32(1) - r2), s1 * r2
    ia, ib, ic = tri[t, 0], tri[t, 1], tri[t, 2]
    out = dict(triangles=t.astype(np.int32),
               points=_mix(positions[ia], positions[ib], positions[ic], w0, w1,
                           w2))
    assert out["points"].dtype == positions.dtype
    if vertex_normals is not None:
        vn = np.asarray(vertex_normals)
        out["normals"] = _mix(vn[ia], vn[ib], vn[ic], w0, w1, w2)
    elif triangle_normals is not None:
        out["normals"] = np.asarray(triangle_normals)[t]
    if vertex_colors is not None:
        c = colors_as_float(vertex_colors)
        out["colors"] = _mix(c[ia], c[ib], c[ic], w0, w1, w2)
        assert out["colors"].dtype == F32
    return out


# ---- the per-pair function -------------------------------------------------------
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + \
        x[..., 2] * y[..., 2]


def closest_point_triangle(p, a, b, c):
    """RaycastingScene.cpp:206-274 in float32 on broadcastable {..,3} arrays.
    -> (point {..,3}, u, v, branch): branch 0..6 = a, b, c, ab, ac, bc,
    inside."""
    p, a, b, c = (np.asarray(x, F32) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        zero, one = F32(0), F32(1)
        conds = [
            (d1 <= zero) & (d2 <= zero),
            (d3 >= zero) & (d4 <= d3),
            (d6 >= zero) & (d5 <= d6),
            (vc <= zero) & (d1 >= zero) & (d3 <= zero),
            (vb <= zero) & (d2 >= zero) & (d6 <= zero),
            (va <= zero) & ((d4 - d3) >= zero) & ((d5 - d6) >= zero),
        ]
        v_ab = d1 / (d1 - d3)
        v_ac = d2 / (d2 - d6)
        v_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = one / ((va + vb) + vc)
        v_in, w_in = vb * denom, vc * denom
        shape = np.broadcast(d1, d1).shape
        full = shape + (3,)
        a_, b_, c_ = (np.broadcast_to(x, full) for x in (a, b, c))
        ab_, ac_ = np.broadcast_to(ab, full), np.broadcast_to(ac, full)
        points = [
            a_, b_, c_,
            a_ + v_ab[..., None] * ab_,
            a_ + v_ac[..., None] * ac_,
            b_ + v_bc[..., None] * (c_ - b_),
            (a_ + v_in[..., None] * ab_) + w_in[..., None] * ac_,
        ]
        z, o = np.zeros(shape, F32), np.ones(shape, F32)
        us = [z, o, z, v_ab, z, one - v_bc, v_in]
        vs = [z, z, o, z, v_ac, v_bc, w_in]
        branch = np.full(shape, 6, np.int32)
        for k in range(5, -1, -1):  # the first true condition wins
            branch = np.where(conds[k], k, branch)
        point = np.empty(full, F32)
        u = np.empty(shape, F32)
        v = np.empty(shape, F32)
        for k in range(7):
            sel = branch == k
            point[sel] = np.broadcast_to(points[k], full)[sel]
            u[sel] = np.broadcast_to(us[k], shape)[sel]
            v[sel] = np.broadcast_to(vs[k], shape)[sel]
    return point, u, v, branch


def box_d2(q, lo, hi):
    zero = F32(0)
    with np.errstate(all="ignore"):
        g = np.maximum(np.maximum(lo - q, q - hi), zero)
        return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + \
            g[..., 2] * g[..., 2]


def pair_d2(q, a, b, c):
    """-> (d2, point, u, v, e2, b2) of queries against triangles, broadcast."""
    q, a, b, c = (np.asarray(x, F32) for x in (q, a, b, c))
    point, u, v, _ = closest_point_triangle(q, a, b, c)
    with np.errstate(all="ignore"):
        d = q - point
        e2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + \
            d[..., 2] * d[..., 2]
        lo = np.minimum(np.minimum(a, b), c)
        hi = np.maximum(np.maximum(a, b), c)
        b2 = box_d2(q, lo, hi) + np.zeros_like(e2)
        d2 = np.where(np.isnan(e2), e2, np.where(e2 > b2, e2, b2))
    return d2, point, u, v, e2, b2


_CHUNK = 1 << 20  # pairs evaluated at once


def closest_points(positions, triangles, queries):
    """The exhaustive loop. -> dict(points, primitive_ids uint32,
    primitive_uvs, primitive_normals, distance, d2)."""
    pos = np.asarray(positions, F32)
    tri = np.asarray(triangles, np.int64)
    queries = np.asarray(queries, F32).reshape(-1, 3)
    a, b, c = pos[tri[:, 0]], pos[tri[:, 1]], pos[tri[:, 2]]
    nq, m = len(queries), len(tri)
    out = dict(points=np.zeros((nq, 3), F32),
               primitive_ids=np.full(nq, NO_TRIANGLE, np.uint32),
               primitive_uvs=np.zeros((nq, 2), F32),
               primitive_normals=np.zeros((nq, 3), F32),
               distance=np.full(nq, np.inf, F32),
               d2=np.full(nq, np.inf, F32))
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        n = np.empty((m, 3), F32)
        n[:, 0] = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n[:, 1] = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        n[:, 2] = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        norm = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) +
                       n[:, 2] * n[:, 2])
        ok = norm > 0
        n[ok] = n[ok] / norm[ok][:, None]
    rows = max(1, _CHUNK // m)
    for s in range(0, nq, rows):
        qs = queries[s:s + rows]
        d2, point, u, v, _, _ = pair_d2(qs[:, None, :], a[None], b[None],
                                        c[None])
        valid = ~np.isnan(d2)
        key = np.where(valid, d2, F32(np.inf))
        best = key.min(axis=1)
        for r in range(len(qs)):
            # the lowest index among the valid pairs at the minimum
            hit = np.flatnonzero(valid[r] & (d2[r] == best[r]))
            if len(hit) == 0:
                continue
            t = int(hit[0])
            i = s + r
            out["points"][i] = point[r, t]
            out["primitive_ids"][i] = t
            out["primitive_uvs"][i] = (u[r, t], v[r, t])
            out["primitive_normals"][i] = n[t]
            out["d2"][i] = d2[r, t]
    with np.errstate(all="ignore"):
        out["distance"] = np.sqrt(out["d2"])
    return out


# ---- metrics -----------------------------------------------------------------------
def compute_metrics(mesh1, mesh2, metrics, radii, n_sampled_points, seed=0):
    """mesh = (positions float32, triangles). -> (values float32, raw)."""
    s1 = sample(mesh1[0], mesh1[1], n_sampled_points, seed)["points"]
    s2 = sample(mesh2[0], mesh2[1], n_sampled_points, seed + 1)["points"]
    d12 = closest_points(mesh2[0], mesh2[1], s1)["distance"]
    d21 = closest_points(mesh1[0], mesh1[1], s2)["distance"]
    raw = dict(sum=[pm.tree_sum(d12), pm.tree_sum(d21)],
               max=[np.float64(d12.max()), np.float64(d21.max())],
               counts=[pm.counts_below(d12, radii),
                       pm.counts_below(d21, radii)])
    n = n_sampled_points
    return pm.values_from_sums(n, n, raw["sum"], raw["max"], raw["counts"],
                               metrics), raw


# ---- meshes the tests share -------------------------------------------------------
def unit_cube(scale=1.0):
    g = golden()["cube"]
    return (np.array(g["positions"], F32) * F32(scale),
            np.array(g["triangles"], np.int32))
