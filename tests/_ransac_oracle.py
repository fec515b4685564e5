"""Numpy restatement of the RANSAC contract (include/o3d_mi355x.h, "RANSAC on
correspondences", rules 1-6): the plain sequential loop of one thread over the
stateless sample stream, numpy.linalg.svd for the Kabsch step. Independent of
the library: Python integers for the sample function, float64 numpy for the
hypothesis and its checks, and a callback for the per-iteration scores
(default: _oracle.evaluate_registration, the pinned CPU body)."""
import math

import numpy as np

M64 = (1 << 64) - 1
EDGE, DISTANCE, NORMAL = 0, 1, 2


def draw(seed, i, j, n):
    """Rule 1: draw j of iteration i over n correspondences."""
    z = (seed + 0x9E3779B97F4A7C15 * (8 * i + j + 1)) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z * n) >> 64


def samples(seed, first, count, ransac_n, n):
    return np.array([[draw(seed, first + i, j, n) for j in range(ransac_n)]
                     for i in range(count)], np.int64).reshape(count, ransac_n)


def kabsch(s, t):
    """Rule 2 on float64 {n,3} arrays -> (R, t, singular values)."""
    s = np.asarray(s, np.float64)
    t = np.asarray(t, np.float64)
    ms, mt = s.mean(0), t.mean(0)
    H = (t - mt).T @ (s - ms)
    U, S, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))
                 or 1.0])
    R = U @ D @ Vt
    return R, mt - R @ ms, S


def _rel_margin(a, b):
    """How far a is from b, relative to their size."""
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def check_edge_length(s, t, thr):
    """-> (passes, smallest relative margin to the threshold)."""
    ok, margin = True, np.inf
    for a in range(len(s)):
        for b in range(a + 1, len(s)):
            ds = float(np.linalg.norm(s[a] - s[b]))
            dt = float(np.linalg.norm(t[a] - t[b]))
            if ds < dt * thr or dt < ds * thr:
                ok = False
            margin = min(margin, _rel_margin(ds, dt * thr),
                         _rel_margin(dt, ds * thr))
    return ok, margin


def check_distance(s, t, R, tr, thr):
    ok, margin = True, np.inf
    for a in range(len(s)):
        d = float(np.linalg.norm(t[a] - (R @ s[a] + tr)))
        if d > thr:
            ok = False
        margin = min(margin, _rel_margin(d, thr))
    return ok, margin


def check_normal(sn, tn, R, thr):
    if sn is None or tn is None:
        return True, np.inf
    c = math.cos(thr)
    ok, margin = True, np.inf
    for a in range(len(sn)):
        d = float(tn[a] @ (R @ sn[a]))
        if d < c:
            ok = False
        margin = min(margin, abs(d - c))
    return ok, margin


def hypothesis(source, target, corres, sample, checkers=(),
               source_normals=None, target_normals=None):
    """Rules 2 and 3 for one sample (rows of corres) -> dict(T, passed,
    margin, ratio): margin = the smallest relative distance of any compared
    quantity to its threshold (the 1e-12 singular-value test included), ratio
    = second / first singular value."""
    c = corres[np.asarray(sample)]
    s = np.asarray(source, np.float64)[c[:, 0]]
    t = np.asarray(target, np.float64)[c[:, 1]]
    R, tr, S = kabsch(s, t)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, tr
    ratio = S[1] / S[0] if S[0] > 0 else 0.0
    passed = S[0] > 0 and S[1] > 1e-12 * S[0]
    margin = abs(ratio - 1e-12) / max(ratio, 1e-12)
    for kind, thr in checkers:
        if kind == EDGE:
            ok, m = check_edge_length(s, t, thr)
        elif kind == DISTANCE:
            ok, m = check_distance(s, t, R, tr, thr)
        else:
            sn = tn = None
            if source_normals is not None and target_normals is not None:
                sn = np.asarray(source_normals, np.float64)[c[:, 0]]
                tn = np.asarray(target_normals, np.float64)[c[:, 1]]
            ok, m = check_normal(sn, tn, R, thr)
        passed = passed and ok
        margin = min(margin, m)
    return dict(T=T, passed=bool(passed), margin=margin, ratio=ratio)


def move(points, T):
    """Rule 4's motion: T cast to the point dtype, TransformPointsKernel's
    statements in that dtype."""
    p = np.ascontiguousarray(points)
    m = np.asarray(T, np.float64).astype(p.dtype).reshape(16)
    p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
    x = [m[4 * r] * p0 + m[4 * r + 1] * p1 + m[4 * r + 2] * p2 + m[4 * r + 3]
         for r in range(4)]
    return np.stack([x[0] / x[3], x[1] / x[3], x[2] / x[3]], 1)


def corres_inliers(source, target, corres, T, max_distance):
    """Rule 6: correspondences with |T s - t|^2 < max_distance^2, in the
    point dtype."""
    dt = np.asarray(source).dtype
    q = move(np.asarray(source)[corres[:, 0]], T)
    d = q - np.asarray(target)[corres[:, 1]]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r = dt.type(max_distance)
    return int((d2 < r * r).sum())


def is_better(fitness, rmse, best_fitness, best_rmse):
    """RegistrationResult::IsBetterRANSACThan."""
    return fitness > best_fitness or (fitness == best_fitness and
                                      rmse < best_rmse)


def update_bound(est_k, ratio, ransac_n, confidence):
    """Rule 6 in float64 as Registration.cpp:315-324; IEEE semantics for
    log(0) and division by zero."""
    def log(x):
        return -math.inf if x == 0.0 else math.log(x)
    num = log(1.0 - confidence)
    den = log(1.0 - math.pow(ratio, ransac_n))
    if den == 0.0:
        if num == 0.0 or math.isnan(num):
            k = math.nan
        else:
            k = math.copysign(math.inf, num) * math.copysign(1.0, den)
    elif math.isinf(num) and math.isinf(den):
        k = math.nan
    else:
        k = num / den
    if k < 0 or math.isnan(k):
        return est_k
    return math.ceil(k) if k < est_k else est_k


def loop(max_iteration, ransac_n, confidence, passed, score):
    """The sequential loop. passed(i) -> bool (rules 2-3); score(i) ->
    (fitness, inlier_rmse, correspondence inlier ratio) of iteration i (rules
    4, 6). -> dict(best_iteration, num_validations, final_iteration_bound,
    fitness, inlier_rmse)."""
    est_k = max_iteration
    best, bf, br, nval = -1, 0.0, 0.0, 0
    i = 0
    while i < est_k:
        if passed(i):
            nval += 1
            f, r, ratio = score(i)
            if is_better(f, r, bf, br):
                best, bf, br = i, f, r
                est_k = update_bound(est_k, ratio, ransac_n, confidence)
        i += 1
    return dict(best_iteration=best, num_validations=nval,
                final_iteration_bound=est_k, fitness=bf, inlier_rmse=br)


def run(source, target, corres, max_distance, ransac_n=3, checkers=(),
        max_iteration=100000, confidence=0.999, seed=0, source_normals=None,
        target_normals=None, evaluate=None):
    """The whole operator on the CPU (small cases)."""
    if evaluate is None:
        import _oracle as orc
        evaluate = orc.evaluate_registration
    n = corres.shape[0]
    if ransac_n < 3 or n < ransac_n or max_distance <= 0:
        return dict(best_iteration=-1, num_validations=0,
                    final_iteration_bound=max_iteration, fitness=0.0,
                    inlier_rmse=0.0, transformation=np.eye(4))
    cache = {}

    def hyp(i):
        if i not in cache:
            cache.clear()
            cache[i] = hypothesis(source, target, corres,
                                  [draw(seed, i, j, n)
                                   for j in range(ransac_n)], checkers,
                                  source_normals, target_normals)
        return cache[i]

    Ts = {}

    def score(i):
        T = hyp(i)["T"]
        Ts[i] = T
        e = evaluate(source, target, max_distance, T)
        return (e["fitness"], e["inlier_rmse"],
                corres_inliers(source, target, corres, T, max_distance) / n)

    out = loop(max_iteration, ransac_n, confidence,
               lambda i: hyp(i)["passed"], score)
    b = out["best_iteration"]
    out["transformation"] = Ts[b] if b >= 0 else np.eye(4)
    return out
