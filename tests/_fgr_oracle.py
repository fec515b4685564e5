"""Numpy restatement of the Fast Global Registration contract
(include/o3d_mi355x.h, "Fast Global Registration", rules 1-4;
include/o3d_mi355x_host.h, rules 5-6). Independent of the library: Python
integers for the sample function, float64 numpy elementwise arithmetic (one
rounding per operation, no FMA) for the terms, explicit loops for the sum tree,
an explicit Cholesky, math.sin / math.cos."""
import math

import numpy as np

M64 = (1 << 64) - 1
TILE = 256
DEFAULTS = dict(division_factor=1.4, use_absolute_scale=False,
                decrease_mu=True, maximum_correspondence_distance=0.025,
                iteration_number=64, tuple_scale=0.95,
                maximum_tuple_count=1000, tuple_test=True, seed=0)


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


# ---- the sum tree -----------------------------------------------------------
def tile_sum_plain(rows):
    """One tile ({m <= 256, C}) by plain loops: lane l adds rows l, l + 64,
    l + 128, l + 192 to +0.0 (a missing row adds +0.0), then the butterfly."""
    rows = np.asarray(rows, np.float64)
    m, C = rows.shape
    out = np.zeros(C)
    for c in range(C):
        lane = [0.0] * 64
        for l in range(64):
            v = 0.0
            for k in range(4):
                r = l + 64 * k
                v = v + (float(rows[r, c]) if r < m else 0.0)
            lane[l] = v
        for o in (32, 16, 8, 4, 2, 1):
            lane = [lane[l] + lane[l ^ o] for l in range(64)]
        out[c] = lane[0]
    return out


def tile_sums(rows):
    """Every tile of {m, C} at once -> {tiles, C}; the same additions as
    tile_sum_plain, tile by tile."""
    rows = np.asarray(rows, np.float64)
    m, C = rows.shape
    tiles = max(1, -(-m // TILE))
    pad = np.zeros((tiles * TILE, C))
    pad[:m] = rows
    pad = pad.reshape(tiles, 4, 64, C)
    v = np.zeros((tiles, 64, C))
    for k in range(4):
        v = v + pad[:, k]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def sum_levels(rows):
    """Rule 1: tiles of 256 rows, the tile sums the next level's rows, until
    one row is left (at least one level)."""
    cur = tile_sums(rows)
    while cur.shape[0] > 1:
        cur = tile_sums(cur)
    return cur[0]


def sum_tiles_in_order(rows):
    """Rule 4: the tile sums added to +0.0 in tile order."""
    t = tile_sums(rows)
    total = np.zeros(t.shape[1])
    for i in range(t.shape[0]):
        total = total + t[i]
    return total


# ---- rule 1 -----------------------------------------------------------------
def normalize(source, target, use_absolute_scale=False):
    out = {"clouds": [], "means": [], "max_scale": []}
    for pts in (source, target):
        p = np.asarray(pts).astype(np.float64)
        mean = sum_levels(p) / float(p.shape[0])
        d = p - mean
        norm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) +
                       d[:, 2] * d[:, 2])
        out["means"].append(mean)
        out["max_scale"].append(float(norm.max()))
        out["clouds"].append(d)
    scale = max(0.0, out["max_scale"][0], out["max_scale"][1])
    out["scale_global"] = 1.0 if use_absolute_scale else scale
    out["scale_start"] = scale if use_absolute_scale else 1.0
    if not out["scale_global"] > 0:
        raise ValueError("Invalid scale_global")
    out["clouds"] = [c / out["scale_global"] for c in out["clouds"]]
    return out


# ---- rule 2 -----------------------------------------------------------------
def nn1(a, b):
    """o3dmi_internal_feature_nn1's definition: sum_k (a_k - b_k)^2 in float64
    over k in order, NaN as +inf, ties to the lowest index."""
    a = np.asarray(a).astype(np.float64)
    b = np.asarray(b).astype(np.float64)
    d = np.zeros((a.shape[0], b.shape[0]))
    for k in range(a.shape[1]):
        e = a[:, k][:, None] - b[:, k][None, :]
        d = d + e * e
    d = np.where(np.isnan(d), np.inf, d)
    return np.argmin(d, axis=1).astype(np.int64)


def initial_matching(fa, fb):
    ij, ji = nn1(fa, fb), nn1(fb, fa)
    return np.array([(i, ij[i]) for i in range(len(ij)) if ji[ij[i]] == i],
                    np.int64).reshape(-1, 2)


# ---- rule 3 -----------------------------------------------------------------
def draw(seed, t, j, n):
    z = (seed + 0x9E3779B97F4A7C15 * (8 * t + j + 1)) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z * n) >> 64


def _edge(a, b):
    d = a - b
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def tuple_test(first, second, corres, tuple_scale, maximum_tuple_count,
               seed):
    """-> (tuples int64 {3 count, 2}, count, trials upstream would have run).
    Every trial is evaluated, then the sequential loop's early exit is applied:
    the stream is stateless, so this is the loop of one thread."""
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    n = corres.shape[0]
    empty = np.zeros((0, 2), np.int64)
    if n <= 2:
        return empty, 0, 0
    total = 100 * n
    r = np.array([[draw(seed, t, j, n) for j in range(3)]
                  for t in range(total)], np.int64)
    A = np.asarray(first).astype(np.float64)
    B = np.asarray(second).astype(np.float64)
    pa = [A[corres[r[:, j], 0]] for j in range(3)]
    pb = [B[corres[r[:, j], 1]] for j in range(3)]
    ok = np.ones(total, bool)
    for x, y in ((0, 1), (1, 2), (2, 0)):
        li, lj = _edge(pa[x], pa[y]), _edge(pb[x], pb[y])
        ok &= (li * tuple_scale < lj) & (lj < li / tuple_scale)
    passing = np.nonzero(ok)[0]
    kept = passing[:maximum_tuple_count]
    trials = int(kept[-1]) + 1 if len(kept) >= maximum_tuple_count else total
    tuples = corres[r[kept].reshape(-1)] if len(kept) else empty
    return tuples.reshape(-1, 2), len(kept), trials


# ---- rule 4 -----------------------------------------------------------------
def terms(p, q, par):
    """Per correspondence the 27 numbers of the rule: the upper triangle of
    JTJ_c (row-major, 21) then JTr_c (6), from the three Jacobian rows as
    written."""
    n = p.shape[0]
    r = p - q
    temp = par / (((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) +
                   r[:, 2] * r[:, 2]) + par)
    s = temp * temp
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    zero, one = np.zeros(n), np.ones(n)
    J = [np.stack([zero, -z, y, -one, zero, zero], 1),
         np.stack([z, zero, -x, zero, -one, zero], 1),
         np.stack([-y, x, zero, zero, zero, -one], 1)]
    out = np.zeros((n, 27))
    col = 0
    for a in range(6):
        for b in range(a, 6):
            out[:, col] = ((J[0][:, a] * J[0][:, b]) * s +
                           (J[1][:, a] * J[1][:, b]) * s) + \
                (J[2][:, a] * J[2][:, b]) * s
            col += 1
    for a in range(6):
        out[:, col] = ((J[0][:, a] * r[:, 0]) * s +
                       (J[1][:, a] * r[:, 1]) * s) + (J[2][:, a] * r[:, 2]) * s
        col += 1
    return out


def solve(JTJ, JTr):
    """-> x of -JTJ x = JTr by the textbook Cholesky of JTJ, or None."""
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = float(JTJ[j][j])
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not (d > 0.0 and d < math.inf):
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            a = float(JTJ[i][j])
            for k in range(j):
                a = a - L[i][k] * L[j][k]
            L[i][j] = a / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        a = float(JTr[i])
        for k in range(i):
            a = a - L[i][k] * y[k]
        y[i] = a / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        a = y[i]
        for k in range(i + 1, 6):
            a = a - L[k][i] * x[k]
        x[i] = a / L[i][i]
    x = [-v for v in x]
    if not all(math.isfinite(v) for v in x):
        return None
    return x


def vector6_to_matrix(x):
    sa, ca = math.sin(x[0]), math.cos(x[0])
    sb, cb = math.sin(x[1]), math.cos(x[1])
    sc, cc = math.sin(x[2]), math.cos(x[2])
    T = np.eye(4)
    T[0, :3] = [cc * cb, (cc * sb) * sa - sc * ca, (cc * sb) * ca + sc * sa]
    T[1, :3] = [sc * cb, (sc * sb) * sa + cc * ca, (sc * sb) * ca - cc * sa]
    T[2, :3] = [-sb, cb * sa, cb * ca]
    T[:3, 3] = x[3:6]
    return T


def _compose(D, T):
    """delta * trans on the 3x4 part, sums left to right."""
    N = np.eye(4)
    for i in range(3):
        for j in range(3):
            N[i, j] = (D[i, 0] * T[0, j] + D[i, 1] * T[1, j]) + \
                D[i, 2] * T[2, j]
        N[i, 3] = ((D[i, 0] * T[0, 3] + D[i, 1] * T[1, 3]) +
                   D[i, 2] * T[2, 3]) + D[i, 3]
    return N


def optimize(source, target, corres, par, division_factor=1.4,
             decrease_mu=True, maximum_correspondence_distance=0.025,
             iteration_number=64, order=None):
    """Rule 4 on two normalised float64 clouds -> (trans, final par, failed
    solves). `order`: "sequential" sums the terms in a plain running loop
    instead of the tile tree (upstream's shape; for the CPU test only)."""
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    trans = np.eye(4)
    failed = 0
    if corres.shape[0] < 10:
        return trans, par, failed
    p = np.asarray(source, np.float64)[corres[:, 0]]
    q = np.asarray(target, np.float64)[corres[:, 1]].copy()
    for itr in range(iteration_number):
        t27 = terms(p, q, par)
        if order == "sequential":
            tot = np.zeros(27)
            for c in range(t27.shape[0]):
                tot = tot + t27[c]
        else:
            tot = sum_tiles_in_order(t27)
        JTJ = np.zeros((6, 6))
        col = 0
        for a in range(6):
            for b in range(a, 6):
                JTJ[a, b] = JTJ[b, a] = tot[col]
                col += 1
        x = solve(JTJ, tot[21:27])
        if x is None:
            failed += 1
            delta = np.eye(4)
        else:
            delta = vector6_to_matrix(x)
            trans = _compose(delta, trans)
            qx, qy, qz = q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy()
            for i in range(3):
                q[:, i] = ((delta[i, 0] * qx + delta[i, 1] * qy) +
                           delta[i, 2] * qz) + delta[i, 3]
        if decrease_mu and itr % 4 == 0 and \
                par > maximum_correspondence_distance:
            par = par / division_factor
    return trans, par, failed


# ---- rule 5 -----------------------------------------------------------------
def original_scale_inverse(trans, means, scale_global):
    R, t = trans[:3, :3], trans[:3, 3]
    g = np.zeros(3)
    for i in range(3):
        rm = (R[i, 0] * means[1][0] + R[i, 1] * means[1][1]) + \
            R[i, 2] * means[1][2]
        g[i] = ((-rm) + t[i] * scale_global) + means[0][i]
    T = np.eye(4)
    T[:3, :3] = R.T
    for i in range(3):
        T[i, 3] = -((R[0, i] * g[0] + R[1, i] * g[1]) + R[2, i] * g[2])
    return T


# ---- whole calls ------------------------------------------------------------
def _finish(source, target, used, opt, info):
    nrm = normalize(source, target, opt["use_absolute_scale"])
    # rule 4: par starts at scale_global (upstream's call site), not scale_start
    trans, par, failed = optimize(
        nrm["clouds"][0], nrm["clouds"][1], used, nrm["scale_global"],
        opt["division_factor"], opt["decrease_mu"],
        opt["maximum_correspondence_distance"], opt["iteration_number"])
    info.update(n_used=len(used), scale_global=nrm["scale_global"],
                final_par=par, failed_solves=failed, used=used)
    return original_scale_inverse(trans, nrm["means"],
                                  nrm["scale_global"]), info


def fgr_correspondence(source, target, corres, **kw):
    """-> (T, info) of o3dmi_registration_fgr_correspondence, without the
    final evaluate."""
    opt = options(**kw)
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    info = dict(n_initial=len(corres), n_trials=0, n_tuples=0, swapped=0)
    used = corres
    if opt["tuple_test"]:
        used, info["n_tuples"], info["n_trials"] = tuple_test(
            source, target, corres, opt["tuple_scale"],
            opt["maximum_tuple_count"], opt["seed"])
    return _finish(source, target, used, opt, info)


def fgr_feature_matching(source, target, fs, ft, **kw):
    opt = options(**kw)
    info = dict(n_trials=0, n_tuples=0, swapped=0)
    if opt["tuple_test"]:
        if len(source) >= len(target):
            pairs = initial_matching(fs, ft)
            used, info["n_tuples"], info["n_trials"] = tuple_test(
                source, target, pairs, opt["tuple_scale"],
                opt["maximum_tuple_count"], opt["seed"])
        else:  # rule 6
            pairs = initial_matching(ft, fs)
            used, info["n_tuples"], info["n_trials"] = tuple_test(
                target, source, pairs, opt["tuple_scale"],
                opt["maximum_tuple_count"], opt["seed"])
            used = used[:, ::-1].copy()
            info["swapped"] = 1
    else:
        pairs = initial_matching(fs, ft)
        used = pairs
    info["n_initial"] = len(pairs)
    info["pairs"] = pairs
    return _finish(source, target, used, opt, info)


# ---- the standard scene of the tests ----------------------------------------
def rotation(axis, angle):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def scene(n, random_share, seed, noise=0.002, n_corres=None):
    """n source points uniform in a 2 x 1.4 x 0.8 box about the origin; target = the source
    under a rotation of 1.3 rad plus a translation, with Gaussian noise and a
    shuffled row order; one pair per source row (or n_corres rows drawn with
    repeats), a share of them with a random target row. -> (source, target,
    corres, T) with T the source-to-target motion."""
    rng = np.random.RandomState(seed)
    src = rng.uniform(-0.5, 0.5, (n, 3)) * [2.0, 1.4, 0.8]
    T = np.eye(4)
    T[:3, :3] = rotation(rng.normal(size=3), 1.3)
    T[:3, 3] = [0.4, -0.3, 0.6]
    perm = rng.permutation(n)
    tgt = np.zeros((n, 3))
    tgt[perm] = src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, noise, (n, 3))
    rows = np.arange(n) if n_corres is None else rng.randint(0, n, n_corres)
    true = perm[rows]
    rnd = rng.randint(0, n, len(rows))
    bad = rng.uniform(size=len(rows)) < random_share
    corres = np.stack([rows, np.where(bad, rnd, true)], 1).astype(np.int64)
    return src, tgt, corres, T


def pose_error(T, T_true):
    """(rotation angle between the two, norm of the translation difference)."""
    R = T[:3, :3].T @ T_true[:3, :3]
    # |R - I|_F = 2 sqrt(2) sin(angle / 2): well conditioned at 0
    f = np.linalg.norm(R - np.eye(3))
    ang = 2.0 * math.asin(min(1.0, f / (2.0 * math.sqrt(2.0))))
    return ang, float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


def pose_change(T, U):
    """(Frobenius norm of the 3x3 difference, norm of the translation
    difference)."""
    return (float(np.linalg.norm(T[:3, :3] - U[:3, :3])),
            float(np.linalg.norm(T[:3, 3] - U[:3, 3])))
