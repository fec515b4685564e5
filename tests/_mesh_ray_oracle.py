"""numpy float32 restatement of the ray queries on a mesh as
include/o3d_mi355x_host.h pins them, BY EXHAUSTIVE LOOPS OVER ALL (ray,
triangle) PAIRS. It never builds a tree.

  pair      Moeller-Trumbore without contraction, every dot product
            (x x + y y) + z z; a miss when det == 0 or NaN; the slab interval
            [T0, T1] of the triangle's own box with divisions; the pair hits
            iff hit_e && T0 <= T1 && tnear < t_e <= tfar;
            t = min(max(t_e, T0), T1) + 0
  closest   the minimum t over the hitting pairs, the lowest index among equals
  any       whether a pair hits
  count     the number of distinct t among the hitting pairs on (0, +inf]
  list      the distinct t ascending, the lowest index at each
  vote      inside when more than nsamples / 2 of the rays (point, direction j)
            have an odd count; the directions from raw MT19937 output through
            libstdc++'s generate_canonical<float, 24> and the distribution's
            affine map
  pinhole   K^-1 by the adjugate in float64, R^T K^-1 and C = -(R^T t)
            narrowed once, the float rows (m0 px + m1 py) + m2
"""
import json
import os

import numpy as np

import _mesh_distance_oracle as md

F32 = np.float32
INVALID_ID = 0xFFFFFFFF
INF = F32(np.inf)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "raycasting_vectors.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def unit_box():
    """TriangleMesh::CreateBox(): 12 triangles, coincident diagonals."""
    return md.unit_cube()


# ---- the pair ------------------------------------------------------------------
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + \
        x[..., 2] * y[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1],
                     x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def slab(o, d, lo, hi, tnear, tfar):
    """-> (non-empty, T0, T1) of rays o, d {..,3} on boxes lo, hi {..,3}."""
    shape = np.broadcast(o[..., 0], lo[..., 0]).shape
    t0 = np.full(shape, tnear, F32)
    t1 = np.full(shape, tfar, F32)
    inside = np.ones(shape, bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            ok, dk = o[..., k], d[..., k]
            moving = np.broadcast_to(dk != 0, shape)
            a = (lo[..., k] - ok) / dk
            b = (hi[..., k] - ok) / dk
            t0 = np.where(moving, np.maximum(t0, np.minimum(a, b)), t0)
            t1 = np.where(moving, np.minimum(t1, np.maximum(a, b)), t1)
            inside &= moving | ~((ok < lo[..., k]) | (ok > hi[..., k]))
    return inside & (t0 <= t1), t0, t1


def pairs(positions, triangles, rays, tnear=0.0, tfar=np.inf):
    """-> hit {R,M} bool and t, u, v {R,M} float32 of every pair."""
    pos = np.asarray(positions, F32)
    tri = np.asarray(triangles).astype(np.int64)
    rays = np.asarray(rays, F32).reshape(-1, 6)
    tnear, tfar = F32(tnear), F32(tfar)
    a, b, c = (pos[tri[:, k]][None, :, :] for k in range(3))
    o, d = rays[:, None, :3], rays[:, None, 3:]
    with np.errstate(all="ignore"):
        e1, e2, s = b - a, c - a, o - a
        p = _cross(np.broadcast_to(d, s.shape), np.broadcast_to(e2, s.shape))
        det = _dot(np.broadcast_to(e1, s.shape), p)
        valid = (det != 0) & ~np.isnan(det)
        inv = F32(1) / det
        u = _dot(s, p) * inv
        q = _cross(s, np.broadcast_to(e1, s.shape))
        v = _dot(np.broadcast_to(d, s.shape), q) * inv
        te = _dot(np.broadcast_to(e2, s.shape), q) * inv
        hit_e = valid & (u >= 0) & (v >= 0) & (u + v <= F32(1))
        lo = np.minimum(np.minimum(a, b), c)
        hi = np.maximum(np.maximum(a, b), c)
        some, t0, t1 = slab(o, d, lo, hi, tnear, tfar)
        hit = hit_e & some & (te > tnear) & (te <= tfar)
        t = np.minimum(np.maximum(te, t0), t1) + F32(0)
    assert t.dtype == F32 and u.dtype == F32
    return hit, t, u, v


def _chunks(rays, rows=128):
    rays = np.asarray(rays, F32).reshape(-1, 6)
    for start in range(0, len(rays), rows):
        yield start, rays[start:start + rows]


def _normal(pos, tri_row):
    a, b, c = (pos[k] for k in tri_row)
    n = _cross(b - a, c - a)
    norm = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    return n / norm if norm > 0 else n


# ---- the five results --------------------------------------------------------------
def cast_rays(positions, triangles, rays, tnear=0.0, tfar=np.inf):
    pos = np.asarray(positions, F32)
    tri = np.asarray(triangles).astype(np.int64)
    n = len(np.asarray(rays).reshape(-1, 6))
    out = dict(t_hit=np.full(n, INF, F32),
               geometry_ids=np.full(n, INVALID_ID, np.uint32),
               primitive_ids=np.full(n, INVALID_ID, np.uint32),
               primitive_uvs=np.zeros((n, 2), F32),
               primitive_normals=np.zeros((n, 3), F32))
    for start, part in _chunks(rays):
        hit, t, u, v = pairs(pos, tri, part, tnear, tfar)
        for r in range(len(part)):
            ids = np.flatnonzero(hit[r])
            if len(ids) == 0:
                continue
            best = t[r, ids].min()
            win = ids[t[r, ids] == best][0]  # the lowest index
            i = start + r
            out["t_hit"][i] = best
            out["geometry_ids"][i] = 0
            out["primitive_ids"][i] = win
            out["primitive_uvs"][i] = (u[r, win], v[r, win])
            with np.errstate(all="ignore"):
                out["primitive_normals"][i] = _normal(pos, tri[win])
    return out


def occlusions(positions, triangles, rays, tnear=0.0, tfar=np.inf):
    out = []
    for _, part in _chunks(rays):
        hit = pairs(positions, triangles, part, tnear, tfar)[0]
        out.append(hit.any(axis=1))
    return np.concatenate(out) if out else np.zeros(0, bool)


def list_intersections(positions, triangles, rays):
    """-> dict(ray_splits int64 {R+1}, ray_ids int64, t_hit, geometry_ids,
    primitive_ids, primitive_uvs)."""
    splits, ray_ids, t_hit, prim, uvs = [0], [], [], [], []
    for start, part in _chunks(rays):
        hit, t, u, v = pairs(positions, triangles, part)
        for r in range(len(part)):
            ids = np.flatnonzero(hit[r])
            for value in np.unique(t[r, ids]):  # ascending
                win = ids[t[r, ids] == value][0]
                ray_ids.append(start + r)
                t_hit.append(value)
                prim.append(win)
                uvs.append((u[r, win], v[r, win]))
            splits.append(len(t_hit))
    return dict(ray_splits=np.array(splits, np.int64),
                ray_ids=np.array(ray_ids, np.int64),
                t_hit=np.array(t_hit, F32),
                geometry_ids=np.zeros(len(t_hit), np.uint32),
                primitive_ids=np.array(prim, np.uint32),
                primitive_uvs=np.array(uvs, F32).reshape(-1, 2))


def count_intersections(positions, triangles, rays):
    return np.diff(list_intersections(positions, triangles,
                                      rays)["ray_splits"]).astype(np.int32)


# ---- the vote ------------------------------------------------------------------------
def mt19937_words(seed, n):
    """The first n outputs of std::mt19937(seed): RandomState seeds by the
    same init_genrand, and a full-range uint32 draw is the raw word."""
    rs = np.random.RandomState(seed)
    words = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    first = np.random.RandomState(5489).randint(0, 2 ** 32, dtype=np.uint64)
    assert first == 3499211612  # the generator's published first word
    return words


def generate_canonical_f24(words):
    """libstdc++'s std::generate_canonical<float, 24> on a 32-bit engine: one
    word, float(word) / 2^32 in float, a 1 replaced by the float below it."""
    x = words.astype(F32) / F32(2.0 ** 32)
    return np.where(x >= F32(1), np.nextafter(F32(1), F32(0)), x).astype(F32)


def vote_directions(nsamples):
    """-> {nsamples,3} float32: upstream's 3 x nsamples matrix filled in
    column-major order."""
    a, b = F32(-0.001), F32(0.001)
    c = generate_canonical_f24(mt19937_words(42, 3 * nsamples))
    r = c * (b - a) + a
    return (F32(1) + r).astype(F32).reshape(nsamples, 3)


def vote_inside(positions, triangles, points, nsamples=1):
    points = np.asarray(points, F32).reshape(-1, 3)
    dirs = vote_directions(nsamples)
    odd = np.zeros(len(points), np.int64)
    for j in range(nsamples):
        rays = np.concatenate(
            [points, np.broadcast_to(dirs[j], points.shape)], axis=1)
        odd += count_intersections(positions, triangles, rays) & 1
    return odd > nsamples // 2


def compute_occupancy(positions, triangles, points, nsamples=1):
    inside = vote_inside(positions, triangles, points, nsamples)
    return np.where(inside, F32(1), F32(0)).astype(F32)


def compute_signed_distance(positions, triangles, points, nsamples=1):
    points = np.asarray(points, F32).reshape(-1, 3)
    dist = md.closest_points(positions, triangles, points)["distance"]
    inside = vote_inside(positions, triangles, points, nsamples)
    return (dist.astype(F32) * np.where(inside, F32(-1), F32(1))).astype(F32)


# ---- the pinhole rays ----------------------------------------------------------------
def inverse3(k):
    k = [np.float64(x) for x in np.asarray(k, np.float64).reshape(9)]
    c00 = k[4] * k[8] - k[5] * k[7]
    c01 = k[5] * k[6] - k[3] * k[8]
    c02 = k[3] * k[7] - k[4] * k[6]
    det = (k[0] * c00 + k[1] * c01) + k[2] * c02
    with np.errstate(all="ignore"):
        return np.array([
            c00 / det, (k[2] * k[7] - k[1] * k[8]) / det,
            (k[1] * k[5] - k[2] * k[4]) / det,
            c01 / det, (k[0] * k[8] - k[2] * k[6]) / det,
            (k[2] * k[3] - k[0] * k[5]) / det,
            c02 / det, (k[1] * k[6] - k[0] * k[7]) / det,
            (k[0] * k[4] - k[1] * k[3]) / det], np.float64).reshape(3, 3)


def create_rays_pinhole(intrinsic, extrinsic, width, height):
    inv_k = inverse3(intrinsic)
    e = np.asarray(extrinsic, np.float64).reshape(4, 4)
    centre = np.zeros(3, F32)
    m = np.zeros((3, 3), F32)
    for i in range(3):
        r0, r1, r2 = e[0, i], e[1, i], e[2, i]
        centre[i] = F32(-((r0 * e[0, 3] + r1 * e[1, 3]) + r2 * e[2, 3]))
        for j in range(3):
            m[i, j] = F32((r0 * inv_k[0, j] + r1 * inv_k[1, j]) +
                          r2 * inv_k[2, j])
    px = (np.arange(width).astype(F32) + F32(0.5))[None, :]
    py = (np.arange(height).astype(F32) + F32(0.5))[:, None]
    rays = np.zeros((height, width, 6), F32)
    rays[..., :3] = centre
    for k in range(3):
        rays[..., 3 + k] = (m[k, 0] * px + m[k, 1] * py) + m[k, 2]
    return rays


# ---- meshes the tests share ----------------------------------------------------------
def soup(m, seed, degenerate_every=4):
    """m triangles around random centres; every fourth has b == a."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (m, 1, 3))
    pos = (centres + 0.3 * rng.standard_normal((m, 3, 3))).reshape(-1, 3)
    pos = pos.astype(F32)
    if degenerate_every:
        for t in range(1, m, degenerate_every):
            pos[3 * t + 1] = pos[3 * t]
    return pos, np.arange(3 * m, dtype=np.int32).reshape(m, 3)


def aimed_rays(n, seed, reach=1.5, scale=1.0):
    """n rays from origins in [-reach, reach]^3 through points of the
    central cube [-0.7, 0.7]^3, where soup() puts its triangles; the direction
    is the difference times `scale`, not normalised."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-reach, reach, (n, 3))
    d = (rng.uniform(-0.7, 0.7, (n, 3)) - o) * scale
    return np.concatenate([o, d], axis=1).astype(F32)


def grid(n=8, duplicate=False):
    """An n x n grid of quads in the plane z = 0 over [0, 1]^2, two triangles
    each (zero-thickness boxes); with duplicate every triangle twice in a
    row."""
    xs = (np.arange(n + 1) / n).astype(F32)
    pos = np.array([[x, y, 0] for y in xs for x in xs], F32)
    tri = []
    for j in range(n):
        for i in range(n):
            v = j * (n + 1) + i
            tri.append([v, v + 1, v + n + 2])
            tri.append([v, v + n + 2, v + n + 1])
    tri = np.array(tri, np.int32)
    if duplicate:
        tri = np.repeat(tri, 2, axis=0)
    return pos, tri
