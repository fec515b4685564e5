"""numpy oracle of PointCloud::ComputeMetrics and the nearest-point distances
(o3dmi_pointcloud_compute_metrics, o3dmi_pointcloud_nearest_distance,
o3dmi_metrics_from_sums), restating what include/o3d_mi355x_host.h pins:

  d2        ((dx dx) + dy dy) + dz dz, dx = query - point, in the cloud's dtype;
            the minimum over the target, the lowest index among equals
  d         np.sqrt(d2) in the dtype
  sum       float64, consecutive runs of RUN values added in index order
            (np.cumsum adds left to right), the run sums likewise, level by
            level until one value is left
  counts    d < radius, strict; Float32 clouds compare in Float32, Float64
            clouds against the Float32 radius widened
  values    upstream's ComputeMetricsCommon in Float32
"""
import json
import os

import numpy as np

RUN = 512
CHAMFER, HAUSDORFF, FSCORE = 0, 1, 2
METRIC_CODES = {"ChamferDistance": CHAMFER, "HausdorffDistance": HAUSDORFF,
                "FScore": FSCORE}
_CHUNK = 1 << 22  # elements of the distance matrix held at once

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "pointcloud_metrics_reference_vectors.json")


def reference_vectors():
    with open(GOLDEN) as f:
        return json.load(f)


def nearest(queries, target):
    """-> (d2 {q} in the dtype, idx {q} int32) by brute force."""
    assert queries.dtype == target.dtype
    q, n = len(queries), len(target)
    d2 = np.empty(q, queries.dtype)
    idx = np.empty(q, np.int32)
    rows = max(1, _CHUNK // n)
    tx, ty, tz = (np.ascontiguousarray(target[:, a])[None, :] for a in range(3))
    for s in range(0, q, rows):
        qs = queries[s:s + rows]
        dx = qs[:, 0:1] - tx
        m = dx * dx
        dy = qs[:, 1:2] - ty
        m = m + dy * dy
        dz = qs[:, 2:3] - tz
        m = m + dz * dz
        i = np.argmin(m, axis=1)  # the first of equal minima
        idx[s:s + rows] = i
        d2[s:s + rows] = m[np.arange(len(qs)), i]
    return d2, idx


def nearest_distance(queries, target):
    d2, idx = nearest(queries, target)
    return np.sqrt(d2), idx


def tree_sum(d):
    v = np.asarray(d).astype(np.float64)
    assert len(v) >= 1
    while True:
        m = len(v)
        full = m // RUN
        out = np.empty((m + RUN - 1) // RUN, np.float64)
        if full:
            out[:full] = np.cumsum(v[:full * RUN].reshape(full, RUN),
                                   axis=1)[:, -1]
        if m % RUN:
            out[full] = np.cumsum(v[full * RUN:])[-1]
        v = out
        if len(v) == 1:
            return v[0]


def counts_below(d, radii):
    out = []
    for r in radii:
        r32 = np.float32(r)
        bound = r32 if d.dtype == np.float32 else np.float64(r32)
        out.append(int(np.count_nonzero(d < bound)))
    return out


def values_from_sums(n1, n2, sums, maxs, counts, metrics):
    """counts = [counts12, counts21]. -> Float32 array, upstream's arithmetic."""
    f32, f64 = np.float32, np.float64
    mean12 = f32(f64(sums[0]) / f64(n1))
    mean21 = f32(f64(sums[1]) / f64(n2))
    out = []
    for m in metrics:
        if m == CHAMFER:
            out.append(f32(mean21 + mean12))
        elif m == HAUSDORFF:
            out.append(max(f32(f64(maxs[0])), f32(f64(maxs[1]))))
        elif m == FSCORE:
            for c12, c21 in zip(counts[0], counts[1]):
                precision = f32(f64(f32(c12)) * (f64(100.0) / f64(n1)))
                recall = f32(f64(f32(c21)) * (f64(100.0) / f64(n2)))
                fscore = f32(0)
                if f32(precision + recall) > 0:
                    fscore = f32(f32(f32(f32(2) * precision) * recall) /
                                 f32(precision + recall))
                out.append(fscore)
        else:
            raise ValueError("unknown metric code")
    return np.array(out, np.float32)


def raw(points1, points2, radii):
    """-> dict(d12, i12, d21, i21, sum, max, counts) for the two directions."""
    d12, i12 = nearest_distance(points1, points2)
    d21, i21 = nearest_distance(points2, points1)
    return dict(d12=d12, i12=i12, d21=d21, i21=i21,
                sum=[tree_sum(d12), tree_sum(d21)],
                max=[np.float64(d12.max()), np.float64(d21.max())],
                counts=[counts_below(d12, radii), counts_below(d21, radii)])


def compute_metrics(points1, points2, metrics, radii):
    r = raw(points1, points2, radii)
    return values_from_sums(len(points1), len(points2), r["sum"], r["max"],
                            r["counts"], metrics), r
