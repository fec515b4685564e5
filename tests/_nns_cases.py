"""Inputs and the exhaustive reference of the neighbour-search tests
(tests/test_nns_cases_cpu.py, tests/test_nns_dense_gpu.py). numpy only.

The searches under test run a wave per query (csrc/nns.hip: GatherCells,
WaveTopK, FloorSink). The cases here are the smallest that reach what the
room-surface cloud of the older tests does not: more than kCoopCap = 512
accepted candidates for one query (a merge in the middle of a gather, pruned
pushes after it), floor rounds after a merge and with equal distances at the
floor, more queries than the 16384 waves of a launch, distance ties at the
cut, points at exactly the radius and points on cell faces.

Reference: the oracle's exhaustive forms only (oracle/icp_oracle.cpp,
HybridSearchBrute / KnnSearchBrute): every (d2, index) pair of the whole cloud,
sorted. They share no cell logic with the product.

Every builder returns (points, queries, radius), is seeded, and takes the point
dtype and an offset that is added to every coordinate in float64 before the
cast (so float32 coordinates are quantised as in the reference's large-offset
recipe, cpp/tests/core/NearestNeighborSearch.cpp:831-869). The arrays are
cached and read-only."""
import functools

import numpy as np

import _oracle as orc

DTYPES = (np.float32, np.float64)
OFFSETS = {"origin": (0.0, 0.0, 0.0), "far": (1000.0, -1000.0, 1000.0)}

K_COOP_CAP = 512            # csrc/nns.hip kCoopCap
SMALL_INDEX_POINTS = 4096   # csrc/nns.hip kSmallIndexPoints
LAUNCH_WAVES = 16384        # kCUs * 16 workgroups of 4 waves

WAVE_REUSE_DENSE = LAUNCH_WAVES
WAVE_REUSE_SPARSE = 40


def _cast(a64, offset, dtype):
    a = np.asarray(a64, np.float64) + np.asarray(OFFSETS[offset], np.float64)
    out = np.ascontiguousarray(a.astype(dtype))
    out.setflags(write=False)
    return out


def _dt(name):
    return np.dtype(name).type


# ------------------------------------------------------------------ builders
@functools.lru_cache(maxsize=None)
def _dense_cube64(n):
    rng = np.random.default_rng(7)
    pts = np.array([0.3, -0.2, 0.1]) + rng.uniform(-0.5, 0.5, (n, 3))
    qrs = np.concatenate([pts[:200],
                          pts[200:300] + rng.normal(0, 0.01, (100, 3))])
    return pts, qrs


def dense_cube(dtype, offset="origin", radius=0.4, n=5000):
    """n points uniform in the unit cube centred at (0.3, -0.2, 0.1) (negative
    cell coordinates occur); 300 queries: the first 200 points and 100 points
    jittered by N(0, 0.01). n = 5000 > kSmallIndexPoints: the three-launch
    index build."""
    pts, qrs = _dense_cube64(n)
    return _cast(pts, offset, dtype), _cast(qrs, offset, dtype), radius


def dense_cube_small(dtype, offset="origin", radius=0.4):
    """dense_cube with 3000 points: the one-workgroup small-index build."""
    return dense_cube(dtype, offset, radius, 3000)


LATTICE_STEP = 0.0625
LATTICE_QUERIES = np.array([[0.0, 0.0, 0.0],
                            [0.03125, 0.03125, 0.03125],
                            [0.5, 0.5, 0.5],
                            [0.25, 0.0, 0.0]])
# KNN: queries on faces / edges / corners of the lattice (a coordinate of 0 is
# a cell face of every origin-anchored grid, whatever its cell edge) and ten
# lattice extents (1.0) outside it.
LATTICE_KNN_QUERIES = np.array([[0.0, 0.03125, 0.03125],
                                [0.0, 0.0, 0.03125],
                                [-0.5, -0.5, -0.5],
                                [0.0625, 0.0, -0.0625],
                                [0.03125, 0.0, 0.0],
                                [10.5, 0.0, 0.0],
                                [-10.5, -10.5, -10.5],
                                [0.03125, 10.5, 0.0]])


def lattice(dtype, offset="origin", knn_queries=False):
    """(-8..8) * 0.0625 on each axis: 4913 points, every coordinate and every
    d2 exact in float32 (with the offset too: 1000 + j / 16 has 14 bits)."""
    c = np.arange(-8, 9) * LATTICE_STEP
    g = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    q = LATTICE_QUERIES
    if knn_queries:
        q = np.concatenate([q, LATTICE_KNN_QUERIES])
    return _cast(g, offset, dtype), _cast(q, offset, dtype), 0.25


DUP_P = np.array([0.125, 0.25, -0.125])
DUP_Q = DUP_P + np.array([0.03125, 0.0, 0.0])          # |P - Q| = 1/32 < 0.05
DUP_MID = DUP_P + np.array([0.015625, 0.0, 0.0])
DUP_EQUI = DUP_MID + np.array([0.0, 0.0625, 0.0])       # on the bisector plane


def duplicates_groups():
    """Indices of the copies of P and of Q: the copies sit at the even indices
    0, 2, ... 1998, three of every ten of them are Q."""
    slot = np.arange(1000)
    is_q = np.isin(slot % 10, (2, 5, 8))
    return 2 * slot[~is_q], 2 * slot[is_q]


def duplicates(dtype, offset="origin"):
    """700 copies of P and 300 of Q, interleaved with each other and with 1000
    background points 0.5 .. 2 away from P. Queries: P, Q, their midpoint and a
    point on the perpendicular bisector (dyadic coordinates: P and Q are
    equally distant in exact arithmetic, with the offset too)."""
    rng = np.random.default_rng(11)
    ip, iq = duplicates_groups()
    pts = np.empty((2000, 3))
    pts[ip] = DUP_P
    pts[iq] = DUP_Q
    d = rng.normal(size=(1000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts[1::2] = DUP_P + d * rng.uniform(0.5, 2.0, (1000, 1))
    qrs = np.stack([DUP_P, DUP_Q, DUP_MID, DUP_EQUI])
    return _cast(pts, offset, dtype), _cast(qrs, offset, dtype), 0.2


def cell_faces(dtype, offset="origin"):
    """Points on the faces of the index's cells (edge radius * 1.001) and one
    ulp of the point dtype on either side, on one axis (crossed with off-face
    values on the other two) and on all three (edges and corners of cells),
    plus 2000 filler points. The queries are the face points."""
    radius = 0.125
    rng = np.random.default_rng(13)
    dtype = np.dtype(dtype).type
    face = []
    for j in range(-3, 4):
        v = dtype(j * (radius * 1.001))
        face += [np.nextafter(v, dtype(-np.inf)), v,
                 np.nextafter(v, dtype(np.inf))]
    face = np.array(face, np.float64)             # exact: widening only
    off = [(0.03, -0.04), (-0.2, 0.11), (0.3, 0.29)]
    rows = []
    for axis in range(3):
        for f in face:
            for u, v in off:
                p = [u, v]
                p.insert(axis, f)
                rows.append(p)
    for f in face:
        rows.append([f, f, f])
        rows.append([f, -f, f])
    rows = np.array(rows)
    filler = rng.uniform(-0.5, 0.5, (2000, 3))
    pts = np.concatenate([rows, filler])
    return _cast(pts, offset, dtype), _cast(rows, offset, dtype), radius


TIER_SIZES = (600, 40, 600, 600)        # A, B, C, D in index order
TIER_CELLS = ((-1, -1, -1), (0, -1, -1), (0, -1, 0), (0, 0, 0))
TIER_QUERY = np.array([0.1, 0.03, 0.03])


def inward_tiers(dtype, offset="origin"):
    """A neighbourhood that arrives far points first. GatherCells hands the 27
    cells over in the order x + 3 y + 9 z of their offsets, so four groups in
    four cells of rising order reach the list one after the other: A (600
    points, the farthest) fills the buffer and forces the first merge; B (the
    40 nearest) and C (600, nearer than all of A) pass the pruning and force a
    second one; D (600, between B and C) forces a third, into a list that
    holds B: a merge in the middle of a gather whose current list must compete
    again. (Uniform clouds do not get there: after the first merge few
    candidates pass the k-th pair.) Queries: TIER_QUERY and three points
    0.002 around it."""
    radius = 0.2
    rng = np.random.default_rng(29)
    q = TIER_QUERY
    centre = (np.array([-0.03, -0.03, -0.03]), q + [0.0, -0.035, -0.035],
              q + [0.0, -0.12, 0.0], q + [0.0, 0.075, 0.0])
    jitter = (0.01, 0.003, 0.006, 0.006)
    pts = np.concatenate([c + rng.uniform(-j, j, (n, 3))
                          for c, j, n in zip(centre, jitter, TIER_SIZES)])
    qrs = np.concatenate([q[None, :], q + rng.uniform(-0.002, 0.002, (3, 3))])
    return _cast(pts, offset, dtype), _cast(qrs, offset, dtype), radius


def _in_ball(rng, n, r):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (r * rng.uniform(0, 1, (n, 1)) ** (1.0 / 3.0))


def wave_reuse(dtype, offset="origin", sparse_first=False):
    """2000 points: 1000 in a ball of radius 0.05 at the origin, 1000 in a cube
    of side 20 (kept 1 away from the ball; the last 30 of them are ten
    triplets 0.02 across). 16384 queries within 0.02 of the origin (each has
    the whole ball in range) and 40 in the sparse part: ten at a triplet, 15 at
    a single point, 15 where nothing is. More queries than the 16384 waves of
    a launch: the waves that serve a second query come from a dense one to a
    sparse one, or (sparse_first) the other way round."""
    rng = np.random.default_rng(17)
    ball = _in_ball(rng, 1000, 0.05)
    cube = rng.uniform(-10, 10, (1400, 3))
    cube = cube[np.linalg.norm(cube, axis=1) > 1.0][:970]
    seeds = rng.uniform(-9, 9, (10, 3))
    seeds = seeds + np.where(np.linalg.norm(seeds, axis=1, keepdims=True) < 2,
                             4.0, 0.0)
    trip = (seeds[:, None, :] + rng.uniform(-0.01, 0.01, (10, 3, 3))).reshape(
        -1, 3)
    pts = np.concatenate([ball, cube, trip])
    assert pts.shape == (2000, 3)
    dense = _in_ball(rng, WAVE_REUSE_DENSE, 0.02)
    empty = rng.uniform(-10, 10, (15, 3))
    empty = empty + np.where(
        np.linalg.norm(empty, axis=1, keepdims=True) < 2, 4.0, 0.0)
    sparse = np.concatenate([
        seeds + rng.uniform(-0.005, 0.005, (10, 3)),
        cube[:15] + rng.uniform(-0.005, 0.005, (15, 3)),
        empty])
    qrs = np.concatenate([sparse, dense] if sparse_first else [dense, sparse])
    return _cast(pts, offset, dtype), _cast(qrs, offset, dtype), 0.12


def wave_reuse_sparse_rows(sparse_first):
    if sparse_first:
        return np.arange(WAVE_REUSE_SPARSE)
    return WAVE_REUSE_DENSE + np.arange(WAVE_REUSE_SPARSE)


def two_scales(dtype, offset="origin"):
    """KNN only: 3000 points in a ball of radius 1e-3, 3000 in a cube of side
    100, one point at (1e4, 1e4, 1e4). Queries: 100 of each group, the far
    point, (1e6, 0, 0) and a point 5 outside the cube. radius is None."""
    rng = np.random.default_rng(19)
    ball = _in_ball(rng, 3000, 1e-3)
    cube = rng.uniform(-50, 50, (3000, 3))
    far = np.array([[1e4, 1e4, 1e4]])
    pts = np.concatenate([ball, cube, far])
    qrs = np.concatenate([ball[:100], cube[:100], far,
                          [[1e6, 0.0, 0.0]], [[55.0, 0.0, 0.0]]])
    return _cast(pts, offset, dtype), _cast(qrs, offset, dtype), None


def small_cloud(dtype, n):
    """n uniform points (KNN with k = 64 on 65 and on 40 points) and 50
    queries around them."""
    rng = np.random.default_rng(23 + n)
    pts = rng.uniform(-1, 1, (n, 3))
    qrs = np.concatenate([pts[:10], rng.uniform(-2, 2, (40, 3))])
    return _cast(pts, "origin", dtype), _cast(qrs, "origin", dtype), None


BUILDERS = {"dense_cube": dense_cube, "dense_cube_small": dense_cube_small,
            "lattice": lattice, "duplicates": duplicates,
            "cell_faces": cell_faces, "inward_tiers": inward_tiers,
            "wave_reuse": wave_reuse,
            "two_scales": two_scales}


@functools.lru_cache(maxsize=None)
def _case(name, dtype_name, offset, extra):
    return BUILDERS[name](_dt(dtype_name), offset, **dict(extra))


def case(name, dtype, offset="origin", **extra):
    """Cached BUILDERS[name](dtype, offset, **extra)."""
    return _case(name, np.dtype(dtype).name, offset,
                 tuple(sorted(extra.items())))


# ----------------------------------------------------------------- reference
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def exhaustive_radius(points, queries, radius, keep=None):
    """The oracle's exhaustive hybrid search with a cap of the whole cloud, in
    chunks of queries: (idx {q, keep}, d2 {q, keep}, counts {q}) with the
    uncapped in-radius counts; rows ascending by (d2, index), padded with
    -1 / 0. keep = None keeps the largest count (at least one column)."""
    n, q = points.shape[0], queries.shape[0]
    chunk = max(1, (1 << 21) // n)
    parts = []
    for b in range(0, q, chunk):
        idx, d2, cnt = orc.hybrid_search(points, queries[b:b + chunk], radius,
                                         n, brute=True)
        w = keep if keep is not None else None
        parts.append((idx if w is None else idx[:, :w].copy(),
                      d2 if w is None else d2[:, :w].copy(), cnt))
    cnt = np.concatenate([p[2] for p in parts])
    w = keep if keep is not None else max(int(cnt.max()), 1)
    idx = np.concatenate([p[0][:, :w] for p in parts])
    d2 = np.concatenate([p[1][:, :w] for p in parts])
    return _frozen(np.ascontiguousarray(idx), np.ascontiguousarray(d2), cnt)


@functools.lru_cache(maxsize=None)
def _reference(name, dtype_name, offset, extra, keep):
    pts, qrs, radius = _case(name, dtype_name, offset, extra)
    return exhaustive_radius(pts, qrs, radius, keep)


def reference(name, dtype, offset="origin", keep=None, **extra):
    """Cached exhaustive_radius of a case."""
    return _reference(name, np.dtype(dtype).name, offset,
                      tuple(sorted(extra.items())), keep)


def hybrid_rows(ref, k):
    """What HybridSearch(max_knn = k) returns, cut from exhaustive_radius rows
    (k <= their width): the first k columns and min(count, k)."""
    idx, d2, cnt = ref
    assert k <= idx.shape[1] or int(cnt.max()) <= idx.shape[1]
    if k > idx.shape[1]:
        pad = k - idx.shape[1]
        idx = np.concatenate([idx, np.full((idx.shape[0], pad), -1, np.int32)],
                             1)
        d2 = np.concatenate([d2, np.zeros((d2.shape[0], pad), d2.dtype)], 1)
    return (np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(d2[:, :k]),
            np.minimum(cnt, k).astype(np.int32))


def flat_lists(ref):
    """The CSR lists of FixedRadiusSearch from exhaustive_radius rows of full
    width."""
    idx, d2, cnt = ref
    assert int(cnt.max()) <= idx.shape[1]
    keep = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    return idx[keep], d2[keep]


@functools.lru_cache(maxsize=None)
def _knn_reference(name, dtype_name, offset, extra, k):
    pts, qrs, _ = _case(name, dtype_name, offset, extra)
    return _frozen(*orc.knn_search(pts, qrs, k))


def knn_reference(name, dtype, k, offset="origin", **extra):
    return _knn_reference(name, np.dtype(dtype).name, offset,
                          tuple(sorted(extra.items())), k)


def numpy_sorted_pairs(points, query):
    """The plain restatement: d2 = ((dx dx) + dy dy) + dz dz in the point
    dtype with dx = query - point, stable sort by (d2, index)."""
    d = query[None, :] - points
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == points.dtype
    order = np.argsort(d2, kind="stable")
    return d2[order], order.astype(np.int32)


def numpy_radius_rows(points, queries, radius, width):
    """exhaustive_radius restated in numpy (strict d2 < r2, r2 = T(radius)^2 in
    the point dtype)."""
    T = points.dtype.type
    r2 = T(radius) * T(radius)
    q = queries.shape[0]
    idx = np.full((q, width), -1, np.int32)
    d2 = np.zeros((q, width), points.dtype)
    cnt = np.zeros(q, np.int32)
    for i in range(q):
        sd, si = numpy_sorted_pairs(points, queries[i])
        m = sd < r2
        c = int(m.sum())
        cnt[i] = c
        idx[i, :c] = si[m]
        d2[i, :c] = sd[m]
    return idx, d2, cnt


# ------------------------------------------------- covariance reference / bar
def covariance_reference(points, idx_row, count):
    """Covariance of the neighbour set idx_row[:count] in numpy.longdouble:
    (exact {3,3}, S {3,3}) with S the sum of the absolute values of each
    entry's addends (x_i - c_a)(x_i - c_b) about the longdouble centroid."""
    p = points[idx_row[:count]].astype(np.longdouble)
    c = p.sum(0) / np.longdouble(count)
    d = p - c
    prod = d[:, :, None] * d[:, None, :]
    return prod.sum(0) / np.longdouble(count - 1), np.abs(prod).sum(0)


def covariance_bound(exact, S, count, dtype):
    """(count + 8) 2^-53 S / (count - 1), + half an ulp of the exact entry for
    float32 (derivation: test_nns_dense_gpu.py, _check_covariances)."""
    b = (np.longdouble(count + 8) * np.longdouble(2.0) ** -53 * S /
         np.longdouble(count - 1))
    if np.dtype(dtype) == np.float32:
        b = b + np.spacing(np.abs(exact).astype(np.float32)).astype(
            np.longdouble) / 2
    return b
