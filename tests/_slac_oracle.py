"""numpy restatement of the rigid half of t::pipelines::slac:

    GetCorrespondenceSetForPointCloudPair   slac/SLACOptimizer.cpp:85-204
    FillInRigidAlignmentTerm (per edge)     slac/FillInLinearSystemImpl.h:36-100
    FillInRigidAlignmentTerm{CPU,CUDA}      kernel/FillInLinearSystemImpl.h:27-154
    RunRigidOptimizerForFragments           slac/SLACOptimizer.cpp:265-286,369-414

Per-pair terms are np.float32 in the reference's operation order; sums, the
solve and the pose update are float64 (the library's documented difference
from the reference's float32 atomics / float32 gesv).
"""
import math

import numpy as np

import _oracle as orc

F = np.float32


def pose_f32(T):
    return np.asarray(T, np.float64).astype(F)


def _rows(t, x, with_t=True):
    """Each output row t0 x + t1 y + t2 z (+ t3), left to right, float32."""
    out = np.empty_like(x)
    for r in range(3):
        v = t[r, 0] * x[:, 0] + t[r, 1] * x[:, 1]
        v = v + t[r, 2] * x[:, 2]
        if with_t:
            v = v + t[r, 3]
        out[:, r] = v
    return out


def transform_rows(T, x):
    return _rows(pose_f32(T), np.ascontiguousarray(x, F))


def rotate_rows(T, x):
    return _rows(pose_f32(T), np.ascontiguousarray(x, F), with_t=False)


def pair_terms(p, q, n, threshold):
    """p = Ti p_a, q = Tj q_b, n = Ri n_a ({m,3} float32) -> (take {m} bool,
    terms {m,28} float32: 21 lower-triangle J_u J_v in unpack21's order,
    6 J_u r, r r), J {m,6}, r {m}."""
    p, q, n = (np.ascontiguousarray(a, F) for a in (p, q, n))
    r = (p[:, 0] - q[:, 0]) * n[:, 0] + (p[:, 1] - q[:, 1]) * n[:, 1]
    r = r + (p[:, 2] - q[:, 2]) * n[:, 2]
    take = ~(np.abs(r) > F(threshold))
    J = np.stack([-q[:, 2] * n[:, 1] + q[:, 1] * n[:, 2],
                  q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2],
                  -q[:, 1] * n[:, 0] + q[:, 0] * n[:, 1],
                  n[:, 0], n[:, 1], n[:, 2]], 1).astype(F)
    cols = [J[:, j] * J[:, k] for j in range(6) for k in range(j + 1)]
    cols += [J[:, k] * r for k in range(6)]
    cols.append(r * r)
    terms = np.stack(cols, 1)
    assert terms.dtype == F and r.dtype == F
    return take, terms, J, r


def sum_terms(take, terms, reverse=False):
    """29 float64 sums (the 28 terms and the count) and sum |terms| {28}."""
    t = terms[take].astype(np.float64)
    if reverse:
        t = t[::-1]
    # row after row (a reduction over the outer axis is sequential), so the
    # reversed run really adds in the opposite order
    s = np.zeros(29)
    if t.shape[0]:
        s[:28] = np.add.reduce(t, axis=0)
    s[28] = float(t.shape[0])
    return s, np.abs(t).sum(0)


def edge_sums(frag_i, frag_j, corres, T_i, T_j, threshold, reverse=False):
    """frag = (positions, normals). -> (sums29, sum |terms| {28})."""
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    p = transform_rows(T_i, frag_i[0][corres[:, 0]])
    n = rotate_rows(T_i, frag_i[1][corres[:, 0]])
    q = transform_rows(T_j, frag_j[0][corres[:, 1]])
    take, terms, _, _ = pair_terms(p, q, n, threshold)
    return sum_terms(take, terms, reverse)


def full_block(p, q, n, threshold):
    """The 12x12 block, 12 rhs and residual as the reference writes them: the
    12-Jacobian (J, -J), every product J_a J_b formed in float32, exactly
    rounded float64 sums."""
    take, _, J, r = pair_terms(p, q, n, threshold)
    J12 = np.concatenate([J, -J], 1)[take]
    r = r[take]
    A = np.zeros((12, 12))
    b = np.zeros(12)
    for a in range(12):
        for c in range(12):
            A[a, c] = math.fsum((J12[:, a] * J12[:, c]).astype(np.float64))
        b[a] = math.fsum((J12[:, a] * r).astype(np.float64))
    return A, b, math.fsum((r * r).astype(np.float64))


def exact_sums(take, terms):
    """The 29 sums with exactly rounded (order-free) float64 sums."""
    t = terms[take].astype(np.float64)
    return np.array([math.fsum(t[:, k]) for k in range(28)] +
                    [float(t.shape[0])])


def compact_block(sums29):
    A = orc.unpack21(sums29[:21])
    b = np.asarray(sums29[21:27], np.float64)
    return (np.block([[A, -A], [-A, A]]), np.concatenate([b, -b]),
            float(sums29[27]))


def scatter_seam(AtA, Atb, residual, sums29, i, j):
    """The seam's update of a float32 system: entry = f32(prev + f32(sum))."""
    A12, b12, res = compact_block(sums29)
    rows = [6 * i + k for k in range(6)] + [6 * j + k for k in range(6)]
    AtA, Atb, residual = AtA.copy(), Atb.copy(), residual.copy()
    for a in range(12):
        for c in range(12):
            AtA[rows[a], rows[c]] = F(AtA[rows[a], rows[c]] + F(A12[a, c]))
        Atb[rows[a]] = F(Atb[rows[a]] + F(b12[a]))
    residual[0] = F(residual[0] + F(res))
    return AtA, Atb, residual


def correspondence_set(pos_i, pos_j, i, j, T_i, T_j, T_ij, distance_threshold,
                       fitness_threshold):
    """-> dict(corres {C,2} int64, inliers, ratio float32, kept)."""
    pos_i = np.ascontiguousarray(pos_i, F)
    pos_j = np.ascontiguousarray(pos_j, F)
    d = F(distance_threshold)
    moved = orc.transform_points(T_ij, pos_i)
    idx, _, _ = orc.hybrid_search(pos_j, moved, float(d), 1)
    idx = idx[:, 0].astype(np.int64)
    a = np.nonzero(idx != -1)[0].astype(np.int64)
    corres = np.stack([a, idx[a]], 1)
    x = orc.transform_points(T_i, pos_i[corres[:, 0]])
    y = orc.transform_points(T_j, pos_j[corres[:, 1]])
    dd = x - y
    sq = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]
    sq = sq + dd[:, 2] * dd[:, 2]
    inliers = int((sq <= d * d).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = F(inliers) / F(corres.shape[0])
    kept = not ((j != i + 1 and ratio < F(fitness_threshold)) or
                corres.shape[0] == 0)
    return dict(corres=corres, inliers=inliers, ratio=ratio, kept=kept)


def solve_lu(A, b):
    """Partial-pivot LU in float64; None on a zero / non-finite pivot."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    n = A.shape[0]
    for k in range(n):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        best = abs(A[piv, k])
        if not best > 0 or not np.isfinite(best):
            return None
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            b[[k, piv]] = b[[piv, k]]
        l = A[k + 1:, k] / A[k, k]
        A[k + 1:, k + 1:] -= l[:, None] * A[k, k + 1:][None, :]
        b[k + 1:] -= l * b[k]
        A[k + 1:, k] = l
    x = np.zeros(n)
    for k in range(n - 1, -1, -1):
        v = b[k]
        for c in range(k + 1, n):
            v -= A[k, c] * x[c]
        x[k] = v / A[k, k]
    if not np.all(np.isfinite(x)):
        return None
    return x


def matmul4(D, T):
    R = np.zeros((4, 4))
    for r in range(4):
        for c in range(4):
            v = 0.0
            for m in range(4):
                v += D[r, m] * T[m, c]
            R[r, c] = v
    return R


def rigid_optimize(fragments, poses, edges, max_iterations=5,
                   distance_threshold=0.07, fitness_threshold=0.3,
                   reverse=False):
    """fragments: list of (positions, normals) float32; poses: list of 4x4
    float64; edges: list of (i, j, T_ij). -> dict(status, poses, losses, kept,
    n_corres, n_inliers). status 'singular' leaves the poses as they came."""
    N = len(fragments)
    poses = [np.array(T, np.float64) for T in poses]
    sets = []
    for (i, j, T_ij) in edges:
        sets.append(correspondence_set(
            fragments[i][0], fragments[j][0], i, j, poses[i], poses[j], T_ij,
            distance_threshold, fitness_threshold))
    out = dict(status="ok", kept=[s["kept"] for s in sets],
               n_corres=[s["corres"].shape[0] for s in sets],
               n_inliers=[0] * len(edges), losses=[], poses=poses)
    T = [p.copy() for p in poses]
    for _ in range(max_iterations):
        AtA = np.zeros((6 * N, 6 * N))
        rhs = np.zeros(6 * N)
        AtA[np.arange(6), np.arange(6)] = 1e5
        loss = 0.0
        for e, (i, j, _) in enumerate(edges):
            cs = sets[e]["corres"] if sets[e]["kept"] else \
                np.zeros((0, 2), np.int64)
            s, _ = edge_sums(fragments[i], fragments[j], cs, T[i], T[j],
                             distance_threshold, reverse)
            A = orc.unpack21(s[:21])
            bi, bj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
            AtA[bi, bi] += A
            AtA[bj, bj] += A
            AtA[bi, bj] -= A
            AtA[bj, bi] -= A
            rhs[bi] -= s[21:27]
            rhs[bj] += s[21:27]
            loss += s[27]
            out["n_inliers"][e] = int(s[28])
        out["losses"].append(loss)
        x = solve_lu(AtA, rhs)
        if x is None:
            out["status"] = "singular"
            return out
        T = [matmul4(orc.pose_to_transformation(x[6 * k:6 * k + 6]), T[k])
             for k in range(N)]
    out["poses"] = T
    return out


# ---- the test scene: overlapping views of the analytic surface --------------
def surface(n, seed):
    """tests/test_feature_gpu._surface: a bumpy sphere with analytic normals."""
    rng = np.random.RandomState(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    th = np.arctan2(v[:, 1], v[:, 0])
    ph = np.arccos(np.clip(v[:, 2], -1, 1))

    def P(t, f):
        rr = 1.0 + 0.08 * np.sin(5 * t) * np.sin(4 * f) + 0.05 * np.cos(7 * f)
        return np.stack([np.sin(f) * np.cos(t), np.sin(f) * np.sin(t),
                         np.cos(f)], 1) * rr[:, None]
    p = P(th, ph)
    e = 1e-6
    dt_ = (P(th + e, ph) - P(th - e, ph)) / (2 * e)
    dp_ = (P(th, ph + e) - P(th, ph - e)) / (2 * e)
    nrm = np.cross(dp_, dt_)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True) + 1e-300
    nrm *= np.sign((nrm * p).sum(1))[:, None]
    return p, nrm


def _rigid(rng, max_deg, max_t):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = np.deg2rad(max_deg) * rng.uniform(0.5, 1.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    t = rng.normal(size=3)
    T[:3, 3] = t / np.linalg.norm(t) * max_t * rng.uniform(0.5, 1.0)
    return T


def make_scene(n_frag=5, n_sample=90000, seed=11, half_angle_deg=75.0,
               step_deg=50.0, perturb_deg=2.0, perturb_t=0.03):
    """N fragments = views of the surface within half_angle of centres spaced
    step_deg apart on the equator, each with its own sampling and its own
    local frame. Returns (fragments, true poses, perturbed poses, edges):
    odometry edges (k, k + 1) and two loop edges, all carrying the true
    T_ij = T_j^-1 T_i."""
    rng = np.random.RandomState(seed)
    frags, truth = [], []
    for k in range(n_frag):
        p, n = surface(n_sample, seed * 100 + k)
        a = np.deg2rad(step_deg * k)
        c = np.array([np.cos(a), np.sin(a), 0.0])
        keep = (p / np.linalg.norm(p, axis=1, keepdims=True)) @ c >= \
            np.cos(np.deg2rad(half_angle_deg))
        p, n = p[keep], n[keep]
        T = _rigid(rng, 40.0, 0.5)           # fragment frame -> world
        Ti = np.linalg.inv(T)
        frags.append(((p @ Ti[:3, :3].T + Ti[:3, 3]).astype(F),
                      (n @ Ti[:3, :3].T).astype(F)))
        truth.append(T)
    start = [_rigid(rng, perturb_deg, perturb_t) @ T for T in truth]
    pairs = [(k, k + 1) for k in range(n_frag - 1)] + [(0, 2), (2, 4)]
    edges = [(i, j, np.linalg.inv(truth[j]) @ truth[i]) for i, j in pairs]
    return frags, truth, start, edges


def relative_errors(poses, truth):
    """Per node k >= 1: (rotation angle in degrees, translation distance) of
    T_0^-1 T_k against the truth."""
    out = []
    for k in range(1, len(poses)):
        R = np.linalg.inv(poses[0]) @ poses[k]
        G = np.linalg.inv(truth[0]) @ truth[k]
        D = np.linalg.inv(G) @ R
        ang = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2,
                                           -1, 1)))
        out.append((float(ang), float(np.linalg.norm(D[:3, 3]))))
    return out
