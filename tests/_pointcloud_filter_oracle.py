"""numpy restatement (brute force) of PointCloud::SelectByMask / SelectByIndex
and the Remove* filters, t/geometry/PointCloud.cpp:435-494, 650-760, with the
arithmetic the HIP backend documents:

  d2 = ((dx*dx) + dy*dy) + dz*dz, dx = query - point, in the point dtype
  neighbours ascending by (d2, index)
  avg accumulated column by column in the point dtype, then / k' in it
  mean and centred sum with math.fsum (exactly rounded float64)
"""
import math

import numpy as np


def select_by_mask(attrs, mask, invert=False):
    keep = np.asarray(mask, bool) != bool(invert)
    return {k: np.asarray(v)[keep] for k, v in attrs.items()}


def select_by_index(attrs, indices, n, invert=False, remove_duplicates=False):
    indices = np.asarray(indices, np.int64)
    if not invert and not remove_duplicates:
        return {k: np.asarray(v)[indices] for k, v in attrs.items()}
    mask = np.zeros(n, bool)
    mask[indices] = True
    return select_by_mask(attrs, mask, invert)


def non_finite_mask(points, remove_nan=True, remove_inf=True):
    p = np.asarray(points)
    keep = np.ones(p.shape[0], bool)
    if remove_nan:
        keep &= ~np.isnan(p).any(1)
    if remove_inf:
        keep &= ~np.isinf(p).any(1)
    return keep


def duplicate_mask(points):
    """Key = the bytes of the point; the lowest index of a key is kept."""
    p = np.ascontiguousarray(points)
    seen = set()
    keep = np.zeros(p.shape[0], bool)
    for i in range(p.shape[0]):
        key = p[i].tobytes()
        if key not in seen:
            seen.add(key)
            keep[i] = True
    return keep


def squared_distances(points, lo, hi):
    """{hi - lo, N} squared distances of queries [lo, hi) to every point."""
    p = np.asarray(points)
    q = p[lo:hi]
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    return ((dx * dx) + dy * dy) + dz * dz


def radius_mask(points, nb_points, search_radius, chunk=512):
    p = np.asarray(points)
    r = p.dtype.type(search_radius)
    r2 = r * r
    keep = np.zeros(p.shape[0], bool)
    for lo in range(0, p.shape[0], chunk):
        d2 = squared_distances(p, lo, min(lo + chunk, p.shape[0]))
        keep[lo:lo + d2.shape[0]] = (d2 < r2).sum(1) >= nb_points
    return keep


def avg_distances(points, nb_neighbors, chunk=512):
    p = np.asarray(points)
    n = p.shape[0]
    k = min(int(nb_neighbors), n)
    avg = np.zeros(n, p.dtype)
    idx = np.arange(n)
    for lo in range(0, n, chunk):
        d2 = squared_distances(p, lo, min(lo + chunk, n))
        rows = d2.shape[0]
        # ascending by (d2, index): lexsort's last key is the primary one
        order = np.lexsort((np.broadcast_to(idx, d2.shape), d2), axis=1)[:, :k]
        near = np.sqrt(np.take_along_axis(d2, order, 1))
        s = np.zeros(rows, p.dtype)
        for j in range(k):
            s = s + near[:, j]
        avg[lo:lo + rows] = s / p.dtype.type(k)
    return avg


def statistical(points, nb_neighbors, std_ratio):
    """-> dict(avg, mean, std, threshold, mask)."""
    avg = avg_distances(points, nb_neighbors)
    n = avg.shape[0]
    a = avg.astype(np.float64)
    mean = math.fsum(a) / n
    s = math.fsum((a - mean) ** 2)
    std = math.sqrt(s / (n - 1)) if n > 1 else float("nan")
    threshold = mean + std_ratio * std
    return dict(avg=avg, mean=mean, std=std, threshold=threshold,
                mask=a <= threshold)


def guard_band_clear(res, rel=1e-9):
    """No point has |avg_i - threshold| <= rel * threshold: a float64 tree
    sum and fsum then cannot disagree on a mask bit."""
    if not math.isfinite(res["threshold"]):
        return True
    a = res["avg"].astype(np.float64)
    return bool((np.abs(a - res["threshold"]) > rel * res["threshold"]).all())


def exactly_degenerate(res):
    """Every avg_i is the same number a, and n * a is exact (a == 0, which is
    what nb_neighbors = 1 gives, or n <= 2): mean == a and the centred sum
    == 0 in EVERY summation order, so the threshold is a itself on both sides
    and no mask bit can differ although |avg_i - threshold| = 0."""
    a = res["avg"]
    return bool((a == a[0]).all()) and (a[0] == 0 or a.shape[0] <= 2)


# ---- inputs shared by the CPU (guard band) and the GPU tests ------------------
STAT_NB = (1, 20, 64)
STAT_RATIO = (0.5, 2.0)
STAT_SIZES = ("n1", "n2", "n10", "surface")
RADIUS = 0.25
RADIUS_NB = (1, 3, 16)


def stat_cloud(size, dtype):
    from open3d_amd import synthetic
    rng = np.random.RandomState(7)
    if size == "n1":
        p = rng.uniform(-1, 1, (1, 3))
    elif size == "n2":
        p = rng.uniform(-1, 1, (2, 3))
    elif size == "n10":
        p = rng.uniform(-1, 1, (10, 3))
    else:
        s = synthetic.make_icp_pair(2000, 2000, seed=3)["target"]
        s = s.astype(np.float64)
        far = rng.uniform(-1, 1, (20, 3)) * 0.5 + np.array([6.0, 7.0, -5.0])
        dup = s[rng.randint(0, s.shape[0], 30)]
        p = np.concatenate([s, far, dup])
        p = p[rng.permutation(p.shape[0])]
    return np.ascontiguousarray(p.astype(dtype))


def radius_cloud(dtype):
    from open3d_amd import synthetic
    rng = np.random.RandomState(11)
    s = synthetic.make_icp_pair(2000, 2000, seed=5)["target"]
    s = s.astype(np.float64)
    lone = rng.uniform(-1, 1, (12, 3)) * 3 + np.array([-20.0, 15.0, 9.0])
    dup = s[rng.randint(0, s.shape[0], 25)]
    # exactly RADIUS apart (0.25 and its square are exact in both dtypes):
    # d2 == r2, which the strict comparison leaves out
    pair = np.array([[10.0, 10.0, 10.0], [10.0 + RADIUS, 10.0, 10.0]])
    p = np.concatenate([s, lone, dup, pair])
    order = rng.permutation(p.shape[0])
    return np.ascontiguousarray(p[order].astype(dtype)), \
        np.nonzero(order >= p.shape[0] - 2)[0]


def reference_vectors():
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        "pointcloud_filter_reference_vectors.json")
    with open(path) as f:
        return json.load(f)


def f32(rows):
    return np.array([[float(v) for v in r] for r in rows], np.float32)


_AVG = {}


def stat_reference(size, dtype, nb_neighbors, std_ratio):
    """statistical() of stat_cloud(size, dtype); the neighbour search is
    computed once per (size, dtype, nb_neighbors). Results are read-only."""
    key = (size, np.dtype(dtype).name, nb_neighbors)
    if key not in _AVG:
        avg = avg_distances(stat_cloud(size, dtype), nb_neighbors)
        avg.setflags(write=False)
        _AVG[key] = avg
    avg = _AVG[key]
    n = avg.shape[0]
    a = avg.astype(np.float64)
    mean = math.fsum(a) / n
    s = math.fsum((a - mean) ** 2)
    std = math.sqrt(s / (n - 1)) if n > 1 else float("nan")
    threshold = mean + std_ratio * std
    return dict(avg=avg, mean=mean, std=std, threshold=threshold,
                mask=a <= threshold)
