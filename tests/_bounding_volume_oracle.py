"""A plain numpy float64 restatement of o3dmi_pointcloud_oriented_bounding_box
(MINIMAL_APPROX, PCA) and o3dmi_pointcloud_oriented_bounding_ellipsoid
(include/o3d_mi355x_host.h, docs/bounding_volumes.md) on the hull of
_pointcloud_hull_oracle.convex_hull: the same statements in the same order,
every sum in the library's fixed tree (or, on request, in plain index order or
in reverse, which is how the ellipsoid's tolerance is measured). numpy's
element-wise operations round every product and sum on its own, as the library
does without contraction."""
import math

import numpy as np

import _pointcloud_hull_oracle as hull_orc

RUN = 8                 # kBvRun / O3DMI_BV_TREE_RUN
TOLERANCE = 1e-6        # kObeTolerance / O3DMI_OBE_TOLERANCE
MAX_ITERATIONS = 1000   # kObeMaxIterations / O3DMI_OBE_MAX_ITERATIONS
JACOBI_SWEEPS = 8       # eigen3.h: kJacobiSweeps


def hull_of(points):
    """-> (X {V,3} float64: the hull's vertices in ascending point index,
    triangles {T,3} on 0..V-1, point indices {V})."""
    idx, tri = hull_orc.convex_hull(points)
    return np.asarray(points)[idx].astype(np.float64), tri, idx


# ---- the tree -----------------------------------------------------------------------
def tree_sum(values, order="tree"):
    """Sum over axis 0 of {n} or {n,k} float64. "tree": runs of RUN consecutive
    values added in index order from 0.0, the run sums likewise, level by
    level; "index" / "reverse": one running sum in that order."""
    a = np.asarray(values, np.float64)
    a = a.reshape(len(a), -1)
    if order != "tree":
        acc = np.zeros(a.shape[1])
        for row in (a if order == "index" else a[::-1]):
            acc = acc + row
        return acc if np.ndim(values) > 1 else float(acc[0])
    while True:
        pad = (-len(a)) % RUN
        if pad:
            a = np.concatenate([a, np.zeros((pad, a.shape[1]))])
        runs = a.reshape(-1, RUN, a.shape[1])
        acc = np.zeros((runs.shape[0], a.shape[1]))
        for k in range(RUN):
            acc = acc + runs[:, k]
        a = acc
        if len(a) == 1:
            break
    return a[0] if np.ndim(values) > 1 else float(a[0, 0])


def dot3(d, r):
    """((d.x r.x + d.y r.y) + d.z r.z) over the last axis."""
    return (d[..., 0] * r[..., 0] + d[..., 1] * r[..., 1]) + d[..., 2] * r[..., 2]


def _norm(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) +
                   v[..., 2] * v[..., 2])


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


# ---- (a) MINIMAL_APPROX -------------------------------------------------------------
def frames(X, tri):
    """Origin and unit axes of candidates -1 .. T-1 -> a, u, v, w {T+1,3}."""
    a, b, c = X[tri[:, 0]], X[tri[:, 1]], X[tri[:, 2]]
    u, v = b - a, c - a
    w = _cross(u, v)
    v = _cross(w, u)
    with np.errstate(invalid="ignore", divide="ignore"):
        u, v, w = (e / _norm(e)[:, None] for e in (u, v, w))
    eye = np.eye(3)
    return (np.concatenate([np.zeros((1, 3)), a]),
            np.concatenate([eye[0:1], u]), np.concatenate([eye[1:2], v]),
            np.concatenate([eye[2:3], w]))


def minimal_approx(X, tri):
    """-> dict(winner, volumes {T+1} (candidate -1 first), lo, hi, center,
    rotation {3,3}, extent)."""
    a, u, v, w = frames(X, tri)
    lo = np.empty((len(a), 3))
    hi = np.empty((len(a), 3))
    for k in range(0, len(a), 256):
        s = slice(k, k + 256)
        d = X[None, :, :] - a[s, None, :]
        for axis, r in enumerate((u, v, w)):
            c = dot3(d, r[s, None, :])
            lo[s, axis] = c.min(axis=1)
            hi[s, axis] = c.max(axis=1)
    e = hi - lo
    volumes = (e[:, 0] * e[:, 1]) * e[:, 2]
    best = -1
    for k in range(len(volumes)):  # strict <, NaN never wins
        if not math.isnan(volumes[k]) and (
                best < 0 or volumes[k] < volumes[best]):
            best = k
    R = np.stack([u[best], v[best], w[best]], axis=1)
    m = (lo[best] + hi[best]) / 2.0
    center = a[best] + ((R[:, 0] * m[0] + R[:, 1] * m[1]) + R[:, 2] * m[2])
    return dict(winner=best - 1, volumes=volumes, lo=lo[best], hi=hi[best],
                center=center, rotation=R, extent=hi[best] - lo[best])


# ---- the host halves ----------------------------------------------------------------
def jacobi(a):
    """eigen3.h's cyclic Jacobi on a symmetric 3x3 -> (eigenvalues unsorted,
    V with the eigenvectors as columns), statement by statement."""
    a = [[float(a[i][j]) for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(JACOBI_SWEEPS):
        for p in range(2):
            for q in range(p + 1, 3):
                apq = a[p][q]
                if apq == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / \
                    (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * c
                for k in range(3):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p] = c * akp - sn * akq
                    a[k][q] = sn * akp + c * akq
                for k in range(3):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k] = c * apk - sn * aqk
                    a[q][k] = sn * apk + c * aqk
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - sn * vkq
                    V[k][q] = sn * vkp + c * vkq
    return [a[0][0], a[1][1], a[2][2]], V


def _swap(e, V, i, j):
    e[i], e[j] = e[j], e[i]
    for r in range(3):
        V[r][i], V[r][j] = V[r][j], V[r][i]


def frame_from_moments(n, sums):
    """o3dmi_bounding_box_frame_from_moments -> (mean {3}, R {3,3})."""
    c = [float(s) / float(n) for s in sums]
    a = [[0.0] * 3 for _ in range(3)]
    a[0][0] = c[3] - c[0] * c[0]
    a[1][1] = c[6] - c[1] * c[1]
    a[2][2] = c[8] - c[2] * c[2]
    a[0][1] = a[1][0] = c[4] - c[0] * c[1]
    a[0][2] = a[2][0] = c[5] - c[0] * c[2]
    a[1][2] = a[2][1] = c[7] - c[1] * c[2]
    e, V = jacobi(a)
    if e[1] > e[0]:
        _swap(e, V, 1, 0)
    if e[2] > e[0]:
        _swap(e, V, 2, 0)
    if e[2] > e[1]:
        _swap(e, V, 2, 1)
    col = []
    for j in range(2):
        v = [V[0][j], V[1][j], V[2][j]]
        norm = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        v = [x / norm for x in v]
        big = 0
        for r in range(3):
            if abs(v[r]) > abs(v[big]):
                big = r
        if v[big] < 0.0:
            v = [-x for x in v]
        col.append(v)
    col.append([col[0][1] * col[1][2] - col[0][2] * col[1][1],
                col[0][2] * col[1][0] - col[0][0] * col[1][2],
                col[0][0] * col[1][1] - col[0][1] * col[1][0]])
    return np.array(c[:3]), np.array(col).T.copy()


def ldlt_inverse(A):
    """bounding_volume.h's LdltInverse -> the inverse (list of rows), or None
    when a pivot is <= 0 or not finite."""
    n = len(A)
    L = [[0.0] * n for _ in range(n)]
    D = [0.0] * n
    for j in range(n):
        d = float(A[j][j])
        for k in range(j):
            d -= (L[j][k] * L[j][k]) * D[k]
        if not (d > 0.0) or not math.isfinite(d):
            return None
        D[j] = d
        for i in range(j + 1, n):
            v = float(A[i][j])
            for k in range(j):
                v -= (L[i][k] * L[j][k]) * D[k]
            L[i][j] = v / d
    inv = [[0.0] * n for _ in range(n)]
    for c in range(n):
        y = [0.0] * n
        x = [0.0] * n
        for i in range(n):
            v = 1.0 if i == c else 0.0
            for k in range(i):
                v -= L[i][k] * y[k]
            y[i] = v
        for i in range(n - 1, -1, -1):
            v = y[i] / D[i]
            for k in range(i + 1, n):
                v -= L[k][i] * x[k]
            x[i] = v
        for r in range(n):
            inv[r][c] = x[r]
    return inv


PERMUTATIONS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1),
                (2, 1, 0)]


def closest_identity(V, radii):
    """MapOBEToClosestIdentity: the first of the 48 signed permutations of the
    columns with the largest trace -> (R {3,3}, radii {3})."""
    best, pick = -1e9, None
    for p in PERMUTATIONS:
        for bits in range(8):
            s = [1.0 if bits & (1 << k) else -1.0 for k in range(3)]
            score = (s[0] * V[0][p[0]] + s[1] * V[1][p[1]]) + s[2] * V[2][p[2]]
            if score > best:
                best, pick = score, (p, s)
    p, s = pick
    R = np.array([[s[j] * V[r][p[j]] for j in range(3)] for r in range(3)])
    return R, np.array([radii[p[j]] for j in range(3)])


def ellipsoid_from_moments(sums):
    """o3dmi_bounding_ellipsoid_from_moments -> (center, R, radii, Q)."""
    s = [float(x) for x in sums]
    c = s[:3]
    S = [[0.0] * 3 for _ in range(3)]
    S[0][0] = s[3] - c[0] * c[0]
    S[1][1] = s[6] - c[1] * c[1]
    S[2][2] = s[8] - c[2] * c[2]
    S[0][1] = S[1][0] = s[4] - c[0] * c[1]
    S[0][2] = S[2][0] = s[5] - c[0] * c[2]
    S[1][2] = S[2][1] = s[7] - c[1] * c[2]
    inv = ldlt_inverse(S)
    if inv is None:
        raise hull_orc.HullRefused(hull_orc.SINGULAR, "not positive definite")
    Q = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            Q[i][j] = Q[j][i] = inv[i][j] / 3.0
    e, V = jacobi(Q)
    if e[1] < e[0]:
        _swap(e, V, 1, 0)
    if e[2] < e[0]:
        _swap(e, V, 2, 0)
    if e[2] < e[1]:
        _swap(e, V, 2, 1)
    radii = [1.0 / math.sqrt(x) for x in e]
    R, radii = closest_identity(V, radii)
    return np.array(c), R, radii, np.array(Q)


# ---- (b) PCA ------------------------------------------------------------------------
def moments(X, order="tree"):
    """The sums of x, y, z, xx, xy, xz, yy, yz, zz over the vertices."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return tree_sum(np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z,
                              z * z], axis=1), order)


def pca(X):
    """-> dict(sums, mean, lo, hi, center, rotation, extent)."""
    sums = moments(X)
    mean, R = frame_from_moments(len(X), sums)
    d = X - mean[None, :]
    c = np.stack([dot3(d, R[None, :, k]) for k in range(3)], axis=1)
    lo, hi = c.min(axis=0), c.max(axis=0)
    m = (lo + hi) / 2.0
    center = ((R[:, 0] * m[0] + R[:, 1] * m[1]) + R[:, 2] * m[2]) + mean
    return dict(sums=sums, mean=mean, lo=lo, hi=hi, center=center,
                rotation=R, extent=hi - lo)


# ---- (c) Khachiyan's loop -----------------------------------------------------------
def _weighted_terms(X, p):
    px, py, pz = p * X[:, 0], p * X[:, 1], p * X[:, 2]
    return [px, py, pz, px * X[:, 0], px * X[:, 1], px * X[:, 2],
            py * X[:, 1], py * X[:, 2], pz * X[:, 2], p]


def _m_of(X, sums):
    """M_i = [a_i; 1]^T Lambda^-1 [a_i; 1] for the ten sums of Lambda."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    A = [[sums[3], sums[4], sums[5], sums[0]],
         [sums[4], sums[6], sums[7], sums[1]],
         [sums[5], sums[7], sums[8], sums[2]],
         [sums[0], sums[1], sums[2], sums[9]]]
    G = ldlt_inverse(A)
    if G is None:
        raise hull_orc.HullRefused(hull_orc.SINGULAR, "Lambda")
    t = [((G[r][0] * x + G[r][1] * y) + G[r][2] * z) + G[r][3]
         for r in range(4)]
    return ((x * t[0] + y * t[1]) + z * t[2]) + t[3]


def ellipsoid(X, order="tree"):
    """-> dict(iterations, max_m (of the last iteration), final_max_m (of the
    weights the loop ends with, which are the ones Q is made of), sums {9},
    center, rotation, radii, Q)."""
    V = len(X)
    p = np.full(V, 1.0 / float(V))
    dsq = np.zeros(V)
    it, max_m = 0, 0.0
    while True:
        sums = tree_sum(np.stack(_weighted_terms(X, p) + [dsq], axis=1), order)
        if it > 0 and (math.sqrt(sums[10]) <= TOLERANCE or
                       it == MAX_ITERATIONS):
            break
        M = _m_of(X, sums)
        j = int(np.argmax(M))  # the first of the maxima
        max_m = float(M[j])
        step = (max_m - 4.0) / (4.0 * (max_m - 1.0))
        new_p = (1.0 - step) * p
        new_p[j] += step
        d = new_p - p
        dsq = d * d
        p = new_p
        it += 1
    center, R, radii, Q = ellipsoid_from_moments(sums[:9])
    return dict(iterations=it, max_m=max_m,
                final_max_m=float(_m_of(X, sums).max()), sums=sums[:9],
                center=center, rotation=R, radii=radii, Q=Q)


# ---- shapes -------------------------------------------------------------------------
def box_points(center, R, extent):
    """OrientedBoundingBox::GetBoxPoints (BoundingVolume.cpp:190-204)."""
    ax = [R @ (np.eye(3)[k] * (extent[k] / 2.0)) for k in range(3)]
    signs = [(-1, -1, -1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1), (1, 1, 1),
             (-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    return np.array([center + s[0] * ax[0] + s[1] * ax[1] + s[2] * ax[2]
                     for s in signs])


def slack(points):
    """s = 16 * 2^-52 * (the axis-aligned box diagonal + the largest
    |coordinate|): the rounding of a three-term dot of a difference, twice
    over for the centre."""
    P = np.asarray(points, np.float64)
    diag = float(np.linalg.norm(P.max(axis=0) - P.min(axis=0)))
    return 16.0 * 2.0 ** -52 * (diag + float(np.abs(P).max()))
