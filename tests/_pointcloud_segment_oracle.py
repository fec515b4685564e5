"""numpy restatement of PointCloud::ClusterDBSCAN and PointCloud::SegmentPlane
as the library defines them (include/o3d_mi355x_host.h), written from
upstream's sequential loops (geometry/PointCloudCluster.cpp:48-93,
geometry/PointCloudSegmentation.cpp:157-279), not from the kernels.

DBSCAN: brute-force neighbour sets in the point dtype, d2 = ((dx dx) + dy dy)
+ dz dz < eps^2 (strict, eps^2 formed in the point dtype), then upstream's
seed / work-list loop. SegmentPlane: the stateless sample function, both plane
fits, the float64 score in the stated order, the one-thread walk with the
break rule, the final mask and the refit.
"""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "pointcloud_segment_reference_vectors.json")
PLANE_TILE = 512  # points whose d^2 are added in index order before the
#                   tile sums are added in tile order (o3dmi_plane_score)
M64 = (1 << 64) - 1


def reference_vectors():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- DBSCAN --------------------------------------------------------------------
def eps_squared(points, eps):
    r = points.dtype.type(eps)
    return r * r


def neighbour_sets(points, eps, near=None, chunk=256):
    """Ascending index lists of the points with d2 < eps^2, self included.
    Every d2 is evaluated as stated; only pairs whose x alone is out of range
    (|dx| beyond eps with a margin) are left out beforehand. near: a list
    that receives the pairs (i, j), i < j, with |d2 - eps^2| <= 4 ulp."""
    p = np.ascontiguousarray(points)
    n = len(p)
    r2 = eps_squared(p, eps)
    ulp4 = 4.0 * float(np.spacing(r2))
    order = np.argsort(p[:, 0], kind="stable")
    xs = p[order, 0].astype(np.float64)
    reach = float(eps) * (1.0 + 1e-3) + float(np.spacing(np.abs(xs).max()
                                                         if n else 0.0))
    out = [None] * n
    for s in range(0, n, chunk):
        rows = order[s:s + chunk]
        lo = np.searchsorted(xs, xs[s] - reach, "left")
        hi = np.searchsorted(xs, xs[min(n, s + chunk) - 1] + reach, "right")
        cols = order[lo:hi]
        d2 = _d2(p[rows], p[cols])
        hit = d2 < r2
        if near is not None:
            close = np.abs(d2.astype(np.float64) - float(r2)) <= ulp4
            for a, b in zip(*np.nonzero(close)):
                i, j = int(rows[a]), int(cols[b])
                if i < j:
                    near.append((i, j))
        for a, i in enumerate(rows):
            out[int(i)] = np.sort(cols[hit[a]])
    return out


def _d2(q, p):
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    return ((dx * dx) + dy * dy) + dz * dz


def min_gap_ulps(points, eps):
    """Smallest |d2 - eps^2| over all pairs, in ulps of eps^2 (small clouds)."""
    p = np.ascontiguousarray(points)
    r2 = eps_squared(p, eps)
    gap = np.abs(_d2(p, p).astype(np.float64) - float(r2))
    return float(gap.min()) / float(np.spacing(r2)) if gap.size else np.inf


def cluster_dbscan(points, eps, min_points, worklist="stack", nbs=None):
    """PointCloudCluster.cpp:48-93. worklist: "stack" pops the back (as
    upstream), "queue" the front; the labels do not depend on it."""
    n = len(points)
    if nbs is None:
        nbs = neighbour_sets(points, eps)
    labels = np.full(n, -2, np.int32)
    cluster = 0
    for idx in range(n):
        if labels[idx] != -2:
            continue
        if len(nbs[idx]) < min_points:
            labels[idx] = -1
            continue
        labels[idx] = cluster
        work = [int(j) for j in nbs[idx]]
        while work:
            nb = work.pop() if worklist == "stack" else work.pop(0)
            if nb == idx or labels[nb] >= 0:
                continue
            labels[nb] = cluster
            if len(nbs[nb]) >= min_points:
                work.extend(int(q) for q in nbs[nb] if labels[q] < 0)
        cluster += 1
    return labels


# ---- SegmentPlane -----------------------------------------------------------------
def draw(seed, i, j, n):
    """RansacDraw: the counter hash of (seed, i, j) mapped to [0, n)."""
    z = (seed + 0x9E3779B97F4A7C15 * ((i * 8 + j + 1) & M64)) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z * n) >> 64


def plane_sample(seed, i, ransac_n, n):
    """Draw k is uniform over the n - k points not drawn yet, shifted past the
    earlier picks taken in ascending order."""
    picked, out = [], []
    for k in range(ransac_n):
        v = draw(seed, i, k, n - k)
        for earlier in sorted(picked):
            if earlier <= v:
                v += 1
            else:
                break
        picked.append(v)
        out.append(v)
    return out


def _finish(abc, p):
    norm = np.sqrt((abc[0] * abc[0] + abc[1] * abc[1]) + abc[2] * abc[2])
    if norm == 0:
        return np.zeros(4)
    abc = abc / norm
    d = -((abc[0] * p[0] + abc[1] * p[1]) + abc[2] * p[2])
    return np.array([abc[0], abc[1], abc[2], d])


def triangle_plane(p0, p1, p2):
    """TriangleMesh::ComputeTrianglePlane (TriangleMesh.cpp:1248-1262)."""
    e0, e1 = p1 - p0, p2 - p0
    abc = np.array([e0[1] * e1[2] - e0[2] * e1[1],
                    e0[2] * e1[0] - e0[0] * e1[2],
                    e0[0] * e1[1] - e0[1] * e1[0]])
    return _finish(abc, p0)


def plane_from_points(pts):
    """GetPlaneFromPoints (PointCloudSegmentation.cpp:114-155) over the rows
    of pts (float64), sums in row order."""
    c = np.zeros(3)
    for p in pts:
        c = c + p
    c = c / float(len(pts))
    xx = xy = xz = yy = yz = zz = 0.0
    for p in pts:
        r = p - c
        xx += r[0] * r[0]
        xy += r[0] * r[1]
        xz += r[0] * r[2]
        yy += r[1] * r[1]
        yz += r[1] * r[2]
        zz += r[2] * r[2]
    return plane_from_sums(c, xx, xy, xz, yy, yz, zz)


def plane_from_sums(c, xx, xy, xz, yy, yz, zz):
    det_x = yy * zz - yz * yz
    det_y = xx * zz - xz * xz
    det_z = xx * yy - xy * xy
    if det_x > det_y and det_x > det_z:
        abc = np.array([det_x, xz * yz - xy * zz, xy * yz - xz * yy])
    elif det_y > det_z:
        abc = np.array([xz * yz - xy * zz, det_y, xy * xz - yz * xx])
    else:
        abc = np.array([xy * yz - xz * yy, xy * xz - yz * xx, det_z])
    return _finish(abc, c)


def hypothesis(points64, seed, i, ransac_n):
    pick = plane_sample(seed, i, ransac_n, len(points64))
    if ransac_n == 3:
        return triangle_plane(points64[pick[0]], points64[pick[1]],
                              points64[pick[2]])
    return plane_from_points(points64[pick])


def distances(points64, planes):
    """|((a x + b y) + c z) + d|, {b, n}, float64, no FMA."""
    planes = np.atleast_2d(planes)
    x, y, z = points64[:, 0], points64[:, 1], points64[:, 2]
    a, b, c, d = (planes[:, k:k + 1] for k in range(4))
    return np.abs(((a * x + b * y) + c * z) + d)


def plane_score(points64, planes, threshold):
    """counts {b} and the sums of d^2 in the library's tree: index order
    inside tiles of PLANE_TILE points (np.cumsum adds left to right), then
    the tile sums in tile order."""
    planes = np.atleast_2d(planes)
    n = len(points64)
    counts = np.zeros(len(planes), np.int64)
    sums = np.zeros(len(planes))
    for s in range(0, n, PLANE_TILE):
        dist = distances(points64[s:s + PLANE_TILE], planes)
        inl = dist < threshold
        counts += inl.sum(axis=1)
        sums = sums + np.cumsum(np.where(inl, dist * dist, 0.0), axis=1)[:, -1]
    return counts, sums


def break_iteration(fitness, ransac_n, probability, num_iterations):
    if not fitness < 1.0:
        return 0
    den = math.log(1.0 - math.pow(fitness, float(ransac_n)))
    if den == 0:
        return num_iterations
    num = math.log(1.0 - probability) if probability < 1 else -math.inf
    q = num / den
    if not math.isfinite(q) or q < 0:
        return num_iterations
    return int(min(q, float(num_iterations)))


def segment_plane(points, threshold, ransac_n, num_iterations, probability,
                  seed, batch=None):
    """The one-thread walk. batch: hypotheses formed and scored at a time (a
    simulated launch); the result does not depend on it."""
    p64 = np.ascontiguousarray(points, np.float64)
    n = len(p64)
    batch = batch or num_iterations
    best = dict(iteration=-1, fitness=0.0, rmse=0.0, plane=np.zeros(4))
    counted, brk = 0, num_iterations
    first = 0
    while first < num_iterations and counted <= brk:
        count = min(batch, num_iterations - first)
        planes = np.array([hypothesis(p64, seed, first + k, ransac_n)
                           for k in range(count)])
        counts, sums = plane_score(p64, planes, threshold)
        for k in range(count):
            if counted > brk:
                break
            if not planes[k].any():
                continue
            fitness = rmse = 0.0
            if counts[k] > 0:
                fitness = float(counts[k]) / float(n)
                rmse = math.sqrt(float(sums[k]) / float(counts[k]))
            if fitness > best["fitness"] or (fitness == best["fitness"] and
                                             rmse < best["rmse"]):
                best = dict(iteration=first + k, fitness=fitness, rmse=rmse,
                            plane=planes[k])
                brk = break_iteration(fitness, ransac_n, probability,
                                      num_iterations)
            counted += 1
        first += count
    out = dict(best_iteration=best["iteration"], iterations_counted=counted,
               final_break_iteration=brk, fitness=best["fitness"],
               inlier_rmse=best["rmse"], plane=np.zeros(4),
               inliers=np.zeros(0, np.int64))
    if best["iteration"] >= 0:
        inl = np.nonzero(distances(p64, best["plane"])[0] < threshold)[0]
        out["inliers"] = inl.astype(np.int64)
        q = p64[inl]
        c = q.sum(axis=0) / float(len(q))
        r = q - c
        out["plane"] = plane_from_sums(
            c, (r[:, 0] * r[:, 0]).sum(), (r[:, 0] * r[:, 1]).sum(),
            (r[:, 0] * r[:, 2]).sum(), (r[:, 1] * r[:, 1]).sum(),
            (r[:, 1] * r[:, 2]).sum(), (r[:, 2] * r[:, 2]).sum())
    return out
