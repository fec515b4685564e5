"""numpy restatement of the PointCloud smoothing, boundary and normal
orientation loops of t/geometry/kernel/PointCloudImpl.h:229-506, 1339-1753, in
the point dtype: every intermediate is an array of `dtype`, the statements are
upstream's in upstream's order, and sums run over the neighbour list slot by
slot (vectorised over the points, sequential over the slots).

Neighbour lists come from the (d2, index)-ordered brute-force search of
_pointcloud_filter_oracle. Every operator takes a `dtype` argument, so the
same lists can be evaluated in float64.

The boundary test has two tangent frames: upstream's literal one, which tests
|nx - nz| and |ny - nz|, and the one its comment states (|nx| and |ny|), which
is what the library builds.
"""
import json
import math
import os

import numpy as np

import _pointcloud_filter_oracle as flt


# ---- neighbour lists --------------------------------------------------------------
def _sorted_lists(points, k, chunk=512):
    """-> idx {n,k} int64, d2 {n,k}: the k nearest of every point, ascending
    by (d2, index)."""
    p = np.ascontiguousarray(points)
    n = p.shape[0]
    idx = np.zeros((n, k), np.int64)
    d2 = np.zeros((n, k), p.dtype)
    cols = np.arange(n)
    for lo in range(0, n, chunk):
        d = flt.squared_distances(p, lo, min(lo + chunk, n))
        order = np.lexsort((np.broadcast_to(cols, d.shape), d), axis=1)[:, :k]
        idx[lo:lo + d.shape[0]] = order
        d2[lo:lo + d.shape[0]] = np.take_along_axis(d, order, 1)
    return idx, d2


def knn_lists(points, k):
    p = np.asarray(points)
    k = min(int(k), p.shape[0])
    idx, d2 = _sorted_lists(p, k)
    return idx, d2, np.full(p.shape[0], k, np.int64)


def hybrid_lists(points, radius, max_nn):
    """HybridSearch: d2 < r2 (r2 = radius squared in the point dtype), the
    first max_nn kept; idx padded with -1, d2 with 0."""
    p = np.asarray(points)
    n = p.shape[0]
    r = p.dtype.type(radius)
    r2 = r * r
    k = min(int(max_nn), n)
    idx, d2 = _sorted_lists(p, k)
    inside = d2 < r2
    counts = inside.sum(1)
    full_i = np.full((n, int(max_nn)), -1, np.int64)
    full_d = np.zeros((n, int(max_nn)), p.dtype)
    full_i[:, :k] = np.where(inside, idx, -1)
    full_d[:, :k] = np.where(inside, d2, 0)
    return full_i, full_d, counts


def radius_lists(points, radius):
    """FixedRadiusSearch as padded rows (width = the largest count)."""
    p = np.asarray(points)
    cap = min(p.shape[0], 256)
    idx, d2, counts = hybrid_lists(p, radius, cap)
    assert p.shape[0] <= cap or counts.max() < cap, "row wider than the cap"
    w = max(int(counts.max()), 1)
    return idx[:, :w], d2[:, :w], counts


# ---- Laplacian / Taubin --------------------------------------------------------------
def laplacian_pass(points, idx, factor, dtype):
    T = np.dtype(dtype).type
    p = np.asarray(points).astype(dtype)
    n, k = idx.shape
    mean = np.zeros((n, 3), dtype)
    count = np.zeros(n, np.int64)
    rows = np.arange(n)
    for j in range(k):
        nb = idx[:, j]
        ok = (nb >= 0) & (nb != rows)
        mean[ok] = mean[ok] + p[nb[ok]]
        count += ok
    out = p.copy()
    has = count > 0
    inv_count = (1.0 / count[has].astype(np.float64)).astype(dtype)
    alpha = T(factor)
    out[has] = p[has] + alpha * (mean[has] * inv_count[:, None] - p[has])
    return out


def smooth_laplacian(points, iterations, lambda_, max_nn, fixed, dtype,
                     mu=None):
    """SmoothLaplacian, or SmoothTaubin when mu is given."""
    p = np.asarray(points).astype(dtype)
    if p.shape[0] == 0 or iterations == 0 or max_nn <= 0:
        return p.copy()
    k = min(p.shape[0], max_nn + 1)
    table = knn_lists(p, k)[0] if fixed else None
    cur = p
    for _ in range(iterations):
        for f in (lambda_,) if mu is None else (lambda_, mu):
            idx = table if fixed else knn_lists(cur, k)[0]
            cur = laplacian_pass(cur, idx, f, dtype)
    return cur


# ---- MLS -------------------------------------------------------------------------------
def _pinned_sign(v):
    """Last non-zero component positive (the library's rule)."""
    v = v.copy()
    for r in range(v.shape[0]):
        for c in (2, 1, 0):
            if v[r, c] != 0:
                if v[r, c] < 0:
                    v[r] = -v[r]
                break
    return v


def _normalize_rows(nrm, dtype):
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    norm = np.sqrt(x * x + y * y + z * z)
    out = nrm.copy()
    ok = norm > 0
    out[ok] = nrm[ok] / norm[ok, None]
    return out


def smooth_mls(points, normals, idx, d2, counts, radius, dtype):
    """-> dict(points, normals (or None), fitted {n} bool, gap {n}): `gap` is
    (second smallest - smallest eigenvalue) / largest of the float64
    covariance, for the points that were fitted (else inf)."""
    T = np.dtype(dtype).type
    p = np.asarray(points).astype(dtype)
    n = p.shape[0]
    d2 = np.asarray(d2).astype(dtype)
    inv_radius2 = T(1.0 / (radius * radius)) if radius > 0.0 else T(0.0)
    out = p.copy()
    nrm_out = None if normals is None else np.asarray(normals).astype(dtype)
    few = counts < 3
    if nrm_out is not None:
        nrm_out[few] = _normalize_rows(nrm_out[few], dtype)
    centroid = np.zeros((n, 3), dtype)
    weight_sum = np.zeros(n, dtype)
    w = np.exp(-d2 * inv_radius2).astype(dtype)
    width = idx.shape[1]
    for j in range(width):
        nb = idx[:, j]
        ok = (j < counts) & (nb >= 0) & ~few
        centroid[ok] = centroid[ok] + w[ok, j, None] * p[nb[ok]]
        weight_sum[ok] = weight_sum[ok] + w[ok, j]
    fitted = ~few & (weight_sum > 0)
    centroid[fitted] = centroid[fitted] / weight_sum[fitted, None]
    cov = np.zeros((n, 6), dtype)  # xx xy xz yy yz zz
    for j in range(width):
        nb = idx[:, j]
        ok = (j < counts) & (nb >= 0) & fitted
        q = p[nb[ok]] - centroid[ok]
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        wj = w[ok, j]
        cov[ok, 0] = cov[ok, 0] + wj * x * x
        cov[ok, 1] = cov[ok, 1] + wj * x * y
        cov[ok, 2] = cov[ok, 2] + wj * x * z
        cov[ok, 3] = cov[ok, 3] + wj * y * y
        cov[ok, 4] = cov[ok, 4] + wj * y * z
        cov[ok, 5] = cov[ok, 5] + wj * z * z
    gap = np.full(n, np.inf)
    f = np.nonzero(fitted)[0]
    if f.size:
        c = cov[f].astype(np.float64)
        m = np.empty((f.size, 3, 3))
        m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = c[:, 0], c[:, 1], c[:, 2]
        m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = c[:, 1], c[:, 3], c[:, 4]
        m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = c[:, 2], c[:, 4], c[:, 5]
        vals, vecs = np.linalg.eigh(m)
        top = np.maximum(np.abs(vals).max(1), np.finfo(np.float64).tiny)
        gap[f] = (vals[:, 1] - vals[:, 0]) / top
        normal = _pinned_sign(vecs[:, :, 0]).astype(dtype)
        d = p[f] - centroid[f]
        projection = d[:, 0] * normal[:, 0] + d[:, 1] * normal[:, 1] + \
            d[:, 2] * normal[:, 2]
        out[f] = p[f] - projection[:, None] * normal
        if nrm_out is not None:
            nrm_out[f] = normal
    return dict(points=out, normals=nrm_out, fitted=fitted, gap=gap)


def mls_lists(points, radius, max_nn):
    """The neighbourhood mode SmoothMLS picks."""
    if radius > 0.0 and max_nn > 0:
        return hybrid_lists(points, radius, max_nn)
    if max_nn > 0:
        idx, d2, counts = knn_lists(points, max_nn)
        return idx, np.zeros_like(d2), counts
    return radius_lists(points, radius)


# ---- bilateral ---------------------------------------------------------------------------
def smooth_bilateral(points, normals, idx, d2, counts, sigma_s, sigma_r,
                     dtype):
    T = np.dtype(dtype).type
    p = np.asarray(points).astype(dtype)
    nrm = np.asarray(normals).astype(dtype)
    d2 = np.asarray(d2).astype(dtype)
    n = p.shape[0]
    inv_sigma_s2 = T(1.0 / (2.0 * sigma_s * sigma_s))
    inv_sigma_r2 = T(1.0 / (2.0 * sigma_r * sigma_r))
    nx, ny, nz = nrm[:, 0].copy(), nrm[:, 1].copy(), nrm[:, 2].copy()
    normal_norm = np.sqrt(nx * nx + ny * ny + nz * nz)
    live = (counts > 1) & (normal_norm > 0)
    safe = np.where(normal_norm > 0, normal_norm, T(1))
    nx, ny, nz = nx / safe, ny / safe, nz / safe
    weighted = np.zeros((n, 3), dtype)
    weight_sum = np.zeros(n, dtype)
    for j in range(idx.shape[1]):
        nb = idx[:, j]
        ok = (j < counts) & (nb >= 0) & live
        q = p[nb[ok]]
        rd = (p[ok, 0] - q[:, 0]) * nx[ok] + (p[ok, 1] - q[:, 1]) * ny[ok] + \
            (p[ok, 2] - q[:, 2]) * nz[ok]
        wj = np.exp(-d2[ok, j] * inv_sigma_s2 - rd * rd * inv_sigma_r2)
        wj = wj.astype(dtype)
        weighted[ok] = weighted[ok] + wj[:, None] * q
        weight_sum[ok] = weight_sum[ok] + wj
    out = p.copy()
    moved = live & (weight_sum > 0)
    out[moved] = weighted[moved] / weight_sum[moved, None]
    return out


# ---- boundary -----------------------------------------------------------------------------
def plane_frame(normals, dtype, literal):
    """GetCoordinateSystemOnPlane -> (u, v). literal: upstream's test on
    |nx - nz|, |ny - nz|; else the rule its comment states."""
    T = np.dtype(dtype).type
    q = np.asarray(normals).astype(dtype)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    if literal:
        first = ~(np.abs(x - z).astype(np.float64) < 1e-6) | \
            ~(np.abs(y - z).astype(np.float64) < 1e-6)
    else:
        first = ~(np.abs(x).astype(np.float64) < 1e-6) | \
            ~(np.abs(y).astype(np.float64) < 1e-6)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_a = (1.0 / np.sqrt(x * x + y * y).astype(np.float64)).astype(dtype)
        inv_b = (1.0 / np.sqrt(y * y + z * z).astype(np.float64)).astype(dtype)
        v = np.zeros_like(q)
        v[:, 0] = np.where(first, T(-1) * y * inv_a, T(0))
        v[:, 1] = np.where(first, x * inv_a, T(-1) * z * inv_b)
        v[:, 2] = np.where(first, T(0), y * inv_b)
        u = np.empty_like(q)
        u[:, 0] = y * v[:, 2] - z * v[:, 1]
        u[:, 1] = z * v[:, 0] - x * v[:, 2]
        u[:, 2] = x * v[:, 1] - y * v[:, 0]
    return u, v


def boundary(points, normals, idx, counts, angle_threshold, dtype,
             literal=False):
    """-> (mask {n} bool, max_gap {n} in `dtype`; NaN angles -> gap NaN and
    mask False, count - 1 <= 0 -> gap 0)."""
    p = np.asarray(points).astype(dtype)
    n = p.shape[0]
    u, v = plane_frame(normals, dtype, literal)
    width = idx.shape[1]
    angles = np.full((n, width), np.inf, dtype)
    with np.errstate(invalid="ignore"):
        for j in range(1, width):
            nb = idx[:, j]
            ok = (j < counts) & (nb >= 0)
            delta = p[nb[ok]] - p[ok]
            a = v[ok, 0] * delta[:, 0] + v[ok, 1] * delta[:, 1] + \
                v[ok, 2] * delta[:, 2]
            b = u[ok, 0] * delta[:, 0] + u[ok, 1] * delta[:, 1] + \
                u[ok, 2] * delta[:, 2]
            angles[ok, j] = np.arctan2(a, b).astype(dtype)
    m = np.isfinite(angles).sum(1)
    bad = np.isnan(angles).any(1)
    srt = np.sort(np.where(np.isnan(angles), np.inf, angles), axis=1)
    gap = np.zeros(n, dtype)
    for r in np.nonzero((m > 0) & ~bad)[0]:
        a = srt[r, :m[r]]
        g = np.dtype(dtype).type(0)
        if a.size > 1:
            g = max(g, np.diff(a).max())
        wrap = np.dtype(dtype).type(2 * math.pi - float(a[-1]) + float(a[0]))
        gap[r] = max(g, wrap)
    gap[bad] = np.nan
    with np.errstate(invalid="ignore"):
        mask = gap.astype(np.float64) > angle_threshold * math.pi / 180.0
    return mask, gap


# ---- normals -------------------------------------------------------------------------------
def normalize_normals(normals, dtype):
    return _normalize_rows(np.asarray(normals).astype(dtype), dtype)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def orient_to_direction(normals, direction, dtype):
    nrm = np.asarray(normals).astype(dtype)
    d = np.asarray(direction, np.float64).astype(dtype)
    norm = np.sqrt(nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] +
                   nrm[:, 2] * nrm[:, 2])
    out = nrm.copy()
    zero = norm == 0
    out[zero] = d
    flip = ~zero & (_dot(nrm, np.broadcast_to(d, nrm.shape)) < 0)
    out[flip] = nrm[flip] * np.dtype(dtype).type(-1)
    return out


def orient_to_camera(points, normals, camera, dtype):
    p = np.asarray(points).astype(dtype)
    nrm = np.asarray(normals).astype(dtype)
    c = np.asarray(camera, np.float64).astype(dtype)
    ref = c[None, :] - p
    norm = np.sqrt(nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] +
                   nrm[:, 2] * nrm[:, 2])
    out = nrm.copy()
    zero = norm == 0
    norm_new = np.sqrt(ref[:, 0] * ref[:, 0] + ref[:, 1] * ref[:, 1] +
                       ref[:, 2] * ref[:, 2])
    at_camera = zero & (norm_new == 0)
    away = zero & ~at_camera
    out[at_camera] = np.array([0, 0, 1], dtype)
    out[away] = ref[away] / norm_new[away, None]
    flip = ~zero & (_dot(nrm, ref) < 0)
    out[flip] = nrm[flip] * np.dtype(dtype).type(-1)
    return out


# ---- inputs shared by the CPU and the GPU tests -------------------------------------------
def reference_vectors():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        "pointcloud_smooth_reference_vectors.json")
    with open(path) as f:
        return json.load(f)


def laplacian_cloud(n, dtype, kind="surface"):
    """Random clouds without exact distance ties; "dups": 70 copies of one
    point among the others; "offset": the cloud 1000 m away."""
    rng = np.random.RandomState(1000 + n)
    if kind == "dups":
        p = rng.uniform(-1, 1, (n, 3))
        p[5:75] = p[5]
    else:
        p = rng.uniform(-1, 1, (n, 3)) * np.array([1.0, 1.0, 0.2])
    if kind == "offset":
        p = p * 0.5 + np.array([1000.0, -1000.0, 1000.0])
    return np.ascontiguousarray(p.astype(dtype))


SPACING = 0.05
NOISE = 0.2  # sigma, in point spacings


def plane_patch(side, dtype, seed, noise=NOISE, tilt=True):
    """side x side grid of SPACING with Gaussian noise; -> (points, normals)."""
    rng = np.random.RandomState(seed)
    g = np.arange(side) * SPACING
    x, y = np.meshgrid(g, g, indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), np.zeros(side * side)], 1)
    p = p + rng.normal(0, noise * SPACING, p.shape)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (p.shape[0], 1))
    if tilt:
        R = _rotation(np.array([0.3, -0.5, 0.2]))
        p, nrm = p @ R.T, nrm @ R.T
        p = p + np.array([0.7, -0.2, 1.5])
    order = rng.permutation(p.shape[0])
    return (np.ascontiguousarray(p[order].astype(dtype)),
            np.ascontiguousarray(nrm[order].astype(dtype)))


def sphere_patch(n, dtype, seed, noise=NOISE):
    """n points of a Fibonacci sphere cap whose spacing is SPACING."""
    rng = np.random.RandomState(seed)
    total = 4 * n
    radius = SPACING * math.sqrt(total / (4 * math.pi))
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / total
    phi = i * math.pi * (3 - math.sqrt(5))
    s = np.sqrt(1 - z * z)
    unit = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)
    p = unit * radius + rng.normal(0, noise * SPACING, unit.shape)
    order = rng.permutation(n)
    return (np.ascontiguousarray(p[order].astype(dtype)),
            np.ascontiguousarray(unit[order].astype(dtype)))


def sphere_shell(n, dtype):
    """A closed Fibonacci sphere of radius 1 -> (points, outward normals)."""
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    phi = i * math.pi * (3 - math.sqrt(5))
    s = np.sqrt(1 - z * z)
    unit = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)
    return (np.ascontiguousarray(unit.astype(dtype)),
            np.ascontiguousarray(unit.astype(dtype)))


def _rotation(w):
    t = np.linalg.norm(w)
    k = w / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K


def grid_patch(side, dtype, tilt):
    """The boundary scene: an exact side x side grid of SPACING, plus two
    lone points and a pair (count 1 and 2 at 2.5 spacings). The grid is
    jittered by 2 % of the spacing (fixed seed) so that no two angles tie.
    -> (points, normals, rim {n} bool, interior {n} bool)."""
    rng = np.random.RandomState(5)
    g = np.arange(side) * SPACING
    x, y = np.meshgrid(g, g, indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), np.zeros(side * side)], 1)
    ij = np.stack([np.repeat(np.arange(side), side),
                   np.tile(np.arange(side), side)], 1)
    rim = ((ij == 0) | (ij == side - 1)).any(1)
    p[:, :2] += rng.uniform(-0.02, 0.02, (p.shape[0], 2)) * SPACING
    far = side * SPACING + 1.0
    extra = np.array([[far, 0, 0], [0, far, 0], [far, far, 0],
                      [far + SPACING, far, 0]])
    p = np.concatenate([p, extra])
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (p.shape[0], 1))
    is_grid = np.arange(p.shape[0]) < side * side
    rim = np.concatenate([rim, np.zeros(4, bool)])
    if tilt:
        R = _rotation(np.array([0.4, 0.7, -0.3]))
        p, nrm = p @ R.T, nrm @ R.T
    return (np.ascontiguousarray(p.astype(dtype)),
            np.ascontiguousarray(nrm.astype(dtype)), rim, is_grid & ~rim)
