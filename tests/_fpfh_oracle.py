"""numpy restatement of FPFH and CorrespondencesFromFeatures.

Citations are relative to the Open3D source tree:
  pair_feature      t/pipelines/kernel/FeatureImpl.h:25-86 (ComputePairFeature)
  spfh_bins         FeatureImpl.h:88-106 (UpdateSPFHFeature): the bin indices
                    are float64 because of the M_PI literals
  fpfh_from_lists   FeatureImpl.h:108-296 (ComputeFPFHFeature{CPU,CUDA}): the
                    SPFH pass (hist_incr = (scalar_t)(100.0 / (count - 1)),
                    list position 0 skipped) and the FPFH pass (d2 weights,
                    sums in scalar_t in list order, (scalar_t)(100.0 / sum))
  correspondences   t/pipelines/registration/Feature.cpp:279-333, with exact
                    float64 distances and ties to the lowest index (the
                    project's contract; the reference's GPU path leaves
                    near-ties to its GEMM rounding).
Neighbour lists come from tests/_oracle.py (hybrid / KNN) or brute force
(radius only).
"""
import numpy as np

NBINS = 33


def pair_feature(p1, n1, p2, n2, dtype=np.float64):
    """ComputePairFeature on one pair, in `dtype` -> (f0, f1, f2, f3)."""
    T = np.dtype(dtype).type
    p1, n1, p2, n2 = (np.asarray(v, dtype) for v in (p1, n1, p2, n2))
    dp = (p2 - p1).astype(dtype)
    f3 = T(np.sqrt(T(T(dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2])))
    if f3 == 0:
        return (T(0), T(0), T(0), T(0))

    def dot(a, b):
        return T(T(T(a[0] * b[0]) + T(a[1] * b[1])) + T(a[2] * b[2]))

    def cross(a, b):
        return np.array([T(a[1] * b[2]) - T(a[2] * b[1]),
                         T(a[2] * b[0]) - T(a[0] * b[2]),
                         T(a[0] * b[1]) - T(a[1] * b[0])], dtype)

    a1 = T(dot(n1, dp) / f3)
    a2 = T(dot(n2, dp) / f3)
    if np.arccos(np.abs(a1)) > np.arccos(np.abs(a2)):   # :44
        na, nb = n2, n1
        dp = -dp
        f2 = -a2
    else:
        na, nb = n1, n2
        f2 = a1
    v = cross(dp, na)
    vn = T(np.sqrt(T(T(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))
    if vn == 0:
        return (T(0), T(0), T(0), T(0))
    v = (v / vn).astype(dtype)
    w = cross(na, v)
    f1 = dot(v, nb)
    f0 = T(np.arctan2(dot(w, nb), dot(na, nb)))
    return (f0, f1, T(f2), f3)


def spfh_bins(f0, f1, f2):
    """UpdateSPFHFeature's three bins (float64 arithmetic, clamped)."""
    def clamp(h):
        return 10 if h >= 11 else max(0, h)
    h1 = clamp(int(np.floor(11 * (float(f0) + np.pi) / (2.0 * np.pi))))
    h2 = clamp(int(np.floor(11 * (float(f1) + 1.0) * 0.5)))
    h3 = clamp(int(np.floor(11 * (float(f2) + 1.0) * 0.5)))
    return h1, h2, h3


def bin_coords(f0, f1, f2):
    """The unclamped bin coordinates (to flag pairs near a bin edge)."""
    return (11 * (float(f0) + np.pi) / (2.0 * np.pi),
            11 * (float(f1) + 1.0) * 0.5, 11 * (float(f2) + 1.0) * 0.5)


def pair_features(p1, n1, p2, n2, dtype):
    """pair_feature over arrays of pairs {M,3} -> {M,4} (same operations)."""
    dt = np.dtype(dtype)
    p1, n1, p2, n2 = (np.asarray(v, dt) for v in (p1, n1, p2, n2))

    def dot(a, b):
        return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(dt) +
                a[:, 2] * b[:, 2]).astype(dt)

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                         a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                         a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(dt)

    dp = (p2 - p1).astype(dt)
    f3 = np.sqrt(dot(dp, dp)).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        a1 = (dot(n1, dp) / f3).astype(dt)
        a2 = (dot(n2, dp) / f3).astype(dt)
        swap = np.arccos(np.abs(a1)) > np.arccos(np.abs(a2))
        sw = swap[:, None]
        na = np.where(sw, n2, n1)
        nb = np.where(sw, n1, n2)
        dp = np.where(sw, -dp, dp)
        f2 = np.where(swap, -a2, a1).astype(dt)
        v = cross(dp, na)
        vn = np.sqrt(dot(v, v)).astype(dt)
        v = (v / vn[:, None]).astype(dt)
        w = cross(na, v)
        f1 = dot(v, nb)
        f0 = np.arctan2(dot(w, nb), dot(na, nb)).astype(dt)
    zero = (f3 == 0) | (vn == 0)
    out = np.stack([f0, f1, f2, f3], 1).astype(dt)
    out[zero] = 0
    return out


def pair_angles(p1, n1, p2, n2, dtype):
    """The two cosines ComputePairFeature's swap test compares (:44-46), over
    arrays of pairs, in `dtype` (NaN for a coincident pair)."""
    dt = np.dtype(dtype)
    p1, n1, p2, n2 = (np.asarray(v, dt) for v in (p1, n1, p2, n2))

    def dot(a, b):
        return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(dt) +
                a[:, 2] * b[:, 2]).astype(dt)

    dp = (p2 - p1).astype(dt)
    f3 = np.sqrt(dot(dp, dp)).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (dot(n1, dp) / f3).astype(dt), (dot(n2, dp) / f3).astype(dt)


def _bins(f):
    def clamp(h):
        return np.clip(h, 0, 10)
    c = np.stack(bin_coords_v(f), 1)
    return clamp(np.floor(c).astype(np.int64)), c


def bin_coords_v(f):
    f0 = f[:, 0].astype(np.float64)
    f1 = f[:, 1].astype(np.float64)
    f2 = f[:, 2].astype(np.float64)
    return (11 * (f0 + np.pi) / (2.0 * np.pi), 11 * (f1 + 1.0) * 0.5,
            11 * (f2 + 1.0) * 0.5)


def padded(idx, d2, splits):
    """CSR lists -> padded (idx, d2, counts)."""
    counts = np.diff(splits).astype(np.int32)
    w = max(int(counts.max()) if counts.size else 0, 1)
    n = counts.shape[0]
    pi = np.full((n, w), -1, np.int32)
    pd = np.zeros((n, w), d2.dtype)
    col = np.arange(w)[None, :]
    m = col < counts[:, None]
    pi[m] = idx
    pd[m] = d2
    return pi, pd, counts


def fpfh_from_lists(points, normals, idx, d2, counts=None, splits=None,
                    edge_tol=None, list_points=None, out_points=None):
    """Both passes. List row r belongs to point list_points[r] (default r);
    the output has one row per point of out_points (default: every list
    row), whose neighbours must all have list rows. Sums run in list order
    (one neighbour position at a time), in the points dtype. With edge_tol,
    also returns a bool flag per output row: a pair it reads (its own or a
    neighbour's SPFH) has a bin coordinate within edge_tol of an integer."""
    dt = points.dtype
    if splits is not None:
        idx, d2, counts = padded(idx, d2, splits)
    R, W = idx.shape
    lp = np.arange(R) if list_points is None else np.asarray(list_points)
    row_of = np.full(points.shape[0], -1, np.int64)
    row_of[lp] = np.arange(R)
    spfh = np.zeros((R, NBINS), dt)
    edge = np.zeros(R, bool)
    with np.errstate(divide="ignore"):
        incr = np.where(counts > 1,
                        (100.0 / (counts - 1).astype(dt).astype(np.float64)
                         ).astype(dt), 0).astype(dt)
    rr = np.arange(R)
    for i in range(1, W):
        live = np.nonzero(counts > i)[0]
        if live.size == 0:
            break
        q = idx[live, i]
        f = pair_features(points[lp[live]], normals[lp[live]], points[q],
                          normals[q], dt)
        h, c = _bins(f)
        for g in range(3):
            col = h[:, g] + 11 * g
            spfh[live, col] = (spfh[live, col] + incr[live]).astype(dt)
        if edge_tol is not None:
            near = (np.abs(c - np.round(c)) < edge_tol).any(1) & (f[:, 3] != 0)
            edge[live] |= near
    out = rr if out_points is None else row_of[np.asarray(out_points)]
    assert (out >= 0).all()
    O = out.shape[0]
    acc = np.zeros((O, NBINS), dt)
    s = np.zeros((O, 3), dt)
    flagged = edge[out].copy()
    for i in range(1, W):
        live = np.nonzero((counts[out] > i) & (d2[out, i] != 0))[0]
        if live.size == 0:
            continue
        q = row_of[idx[out[live], i]]
        assert (q >= 0).all()
        flagged[live] |= edge[q]
        val = (spfh[q] / d2[out[live], i][:, None]).astype(dt)
        for g in range(3):
            for b in range(11 * g, 11 * g + 11):
                s[live, g] = (s[live, g] + val[:, b]).astype(dt)
        acc[live] = (acc[live] + val).astype(dt)
    with np.errstate(divide="ignore"):
        scale = np.where(s != 0, (100.0 / s.astype(np.float64)), 0).astype(dt)
    fpfh = ((acc * np.repeat(scale, 11, 1)).astype(dt) + spfh[out]).astype(dt)
    fpfh[counts[out] <= 1] = 0
    return (fpfh, flagged) if edge_tol is not None else fpfh


def radius_lists(points, radius):
    """FixedRadiusSearch by brute force: (idx, d2, splits), each row ascending
    by (d2, index), d2 < radius^2 in the points dtype."""
    dt = points.dtype
    T = dt.type
    r2 = T(T(radius) * T(radius))
    idx, dd, splits = [], [], [0]
    for i in range(points.shape[0]):
        d = points - points[i]
        d2 = ((d[:, 0] * d[:, 0]).astype(dt) + (d[:, 1] * d[:, 1]).astype(dt)
              ).astype(dt) + (d[:, 2] * d[:, 2]).astype(dt)
        d2 = d2.astype(dt)
        sel = np.nonzero(d2 < r2)[0]
        order = np.lexsort((sel, d2[sel]))
        sel = sel[order]
        idx.append(sel.astype(np.int32))
        dd.append(d2[sel])
        splits.append(splits[-1] + len(sel))
    return (np.concatenate(idx) if idx else np.zeros(0, np.int32),
            np.concatenate(dd) if dd else np.zeros(0, dt),
            np.array(splits, np.int64))


def feature_distances(a, b):
    """{na, nb} float64 sum_k (a_k - b_k)^2, k ascending."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    d = np.zeros((a.shape[0], b.shape[0]), np.float64)
    for k in range(a.shape[1]):
        x = a[:, k][:, None] - b[:, k][None, :]
        d = d + x * x
    return d


def nn1(a, b, chunk=2048):
    """Nearest row of b for every row of a; ties to the lowest index; a NaN
    distance counts as +inf."""
    out = np.zeros(a.shape[0], np.int64)
    for s in range(0, a.shape[0], chunk):
        with np.errstate(invalid="ignore", over="ignore"):
            d = feature_distances(a[s:s + chunk], b)
        d[np.isnan(d)] = np.inf
        out[s:s + chunk] = np.argmin(d, axis=1)  # argmin: first minimum
    return out


def correspondences(src, tgt, mutual_filter=False, ratio=0.1):
    """CorrespondencesFromFeatures -> (pairs {K,2} int64, fell_back)."""
    ij = nn1(src, tgt)
    ar = np.arange(src.shape[0], dtype=np.int64)
    full = np.stack([ar, ij], 1)
    if not mutual_filter:
        return full, False
    ji = nn1(tgt, src)
    keep = ji[ij] == ar
    if float(keep.sum()) > np.float32(ratio) * np.float32(src.shape[0]):
        return full[keep], False
    return full, True
