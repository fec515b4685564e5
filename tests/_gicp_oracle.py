"""numpy restatement of TransformationEstimationForGeneralizedICP (Segal et
al., "Generalized-ICP", RSS 2009) as the reference's legacy pipeline computes
it (pipelines/registration/GeneralizedICP.cpp), for the generalized ICP tests.
Float64 throughout; the narrowing to the point dtype happens where the clouds'
attributes are stored.

  covariances_from_normals  InitializePointCloudForGeneralizedICP (:33-80), the
                            products spelled as explicit sums in index order
  pair_terms / accumulate   ComputeTransformation up to the solve (:104-147):
                            the 29 sums, the pairs that cannot be whitened,
                            and the sum of |term| per entry
  compute_rmse              ComputeRMSE (:83-102)
  multiscale_icp            DoSingleScaleICPIterations / MultiScaleICP
                            (t/pipelines/registration/Registration.cpp:275-444)
                            with this estimator

W = (Ct + R Cs R^T)^-1/2 comes from np.linalg.eigh over (n,3,3) ("eigh"), or
from a batched cyclic Jacobi ("jacobi"): two routes to the same unique
principal root, whose difference measures the tolerance of the GPU test.
Search, VoxelDownSample, normals, the 6x6 solve and the pose helpers are
_oracle's.
"""
import numpy as np

import _oracle as orc

L2, L1, HUBER, CAUCHY, GM, TUKEY, GENERALIZED = range(7)


def _matmul_in_order(a, b):
    """(n,3,3) x (n,3,3), every entry a_i0 b_0j + a_i1 b_1j + a_i2 b_2j, left
    to right, zero terms included."""
    out = np.empty_like(a)
    for i in range(3):
        for j in range(3):
            out[:, i, j] = (a[:, i, 0] * b[:, 0, j] + a[:, i, 1] * b[:, 1, j] +
                            a[:, i, 2] * b[:, 2, j])
    return out


def covariances_from_normals(normals, epsilon=1e-3):
    """-> {n,3,3} of the normals' dtype; the arithmetic is float64."""
    dt = normals.dtype
    x = np.asarray(normals, np.float64)
    n = x.shape[0]
    e1 = (1.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        v = [e1[1] * x[:, 2] - e1[2] * x[:, 1],
             e1[2] * x[:, 0] - e1[0] * x[:, 2],
             e1[0] * x[:, 1] - e1[1] * x[:, 0]]
        c = e1[0] * x[:, 0] + e1[1] * x[:, 1] + e1[2] * x[:, 2]
        z = np.zeros(n)
        sv = np.empty((n, 3, 3))
        sv[:, 0, 0], sv[:, 0, 1], sv[:, 0, 2] = z, -v[2], v[1]
        sv[:, 1, 0], sv[:, 1, 1], sv[:, 1, 2] = v[2], z, -v[0]
        sv[:, 2, 0], sv[:, 2, 1], sv[:, 2, 2] = -v[1], v[0], z
        factor = 1 / (1 + c)
        eye = np.broadcast_to(np.eye(3), (n, 3, 3))
        Rx = (eye + sv) + _matmul_in_order(sv, sv) * factor[:, None, None]
        # "x and e1 are in the same direction" says the reference; it is the
        # opposite one, and the identity is what it returns
        Rx[c < -0.99] = np.eye(3)
        D = np.broadcast_to(np.diag([epsilon, 1.0, 1.0]), (n, 3, 3)).copy()
        C = _matmul_in_order(_matmul_in_order(Rx, D),
                             np.ascontiguousarray(Rx.transpose(0, 2, 1)))
    return C.astype(dt)


def robust_weight(kernel, r):
    """RobustKernelImpl.h:35-126 on float64 residuals."""
    method, scaling, shape = kernel
    if method == L2:
        return np.ones_like(r)
    with np.errstate(all="ignore"):
        if method == L1:
            return 1.0 / np.abs(r)
        if method == HUBER:
            a = np.abs(r)
            return scaling / np.where(a < scaling, scaling, a)
        if method == CAUCHY:
            q = r / scaling
            return 1.0 / (1.0 + q * q)
        if method == GM:
            s = scaling + r * r
            return scaling / (s * s)
        if method == TUKEY:
            a = np.abs(r) / scaling
            m = np.where(1.0 < a, 1.0, a)
            v = 1.0 - m * m
            return v * v
    flat = np.array([orc.robust_weight(method, scaling, shape, float(x),
                                       f64=True) for x in r.reshape(-1)])
    return flat.reshape(r.shape)


def _sym_from_upper(C):
    """Only the upper triangle of a covariance is read."""
    C = np.asarray(C, np.float64)
    U = np.triu(C)
    return U + np.triu(C, 1).transpose(0, 2, 1)


def jacobi_eigh(M, sweeps=8):
    """Batched cyclic Jacobi of symmetric (n,3,3): rotations in the (0,1),
    (0,2), (1,2) planes, each annihilating that entry, `sweeps` times.
    -> (eigenvalues {n,3} unsorted, eigenvectors in columns {n,3,3})."""
    a = np.array(M, np.float64)
    n = a.shape[0]
    V = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = a[:, p, q]
                skip = apq == 0
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta >= 0, 1.0, -1.0) / (
                    np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                c = np.where(skip, 1.0, c)
                s = np.where(skip, 0.0, s)
                akp, akq = a[:, :, p].copy(), a[:, :, q].copy()
                a[:, :, p] = c[:, None] * akp - s[:, None] * akq
                a[:, :, q] = s[:, None] * akp + c[:, None] * akq
                apk, aqk = a[:, p, :].copy(), a[:, q, :].copy()
                a[:, p, :] = c[:, None] * apk - s[:, None] * aqk
                a[:, q, :] = s[:, None] * apk + c[:, None] * aqk
                vkp, vkq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = c[:, None] * vkp - s[:, None] * vkq
                V[:, :, q] = s[:, None] * vkp + c[:, None] * vkq
    return a[:, [0, 1, 2], [0, 1, 2]], V


def whiten(Cs, Ct, R=None, route="eigh"):
    """W = (Ct + R Cs R^T)^-1/2 per pair -> (W {m,3,3}, ok {m}); ok is False
    where an eigenvalue is not > 0 or not finite."""
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    Cs, Ct = _sym_from_upper(Cs), _sym_from_upper(Ct)
    with np.errstate(all="ignore"):
        M = Ct + R @ Cs @ R.T
        M = np.triu(M) + np.triu(M, 1).transpose(0, 2, 1)
        finite = np.isfinite(M).all(axis=(1, 2))
        Msafe = np.where(finite[:, None, None], M, np.eye(3))
        if route == "eigh":
            lam, V = np.linalg.eigh(Msafe)
        else:
            lam, V = jacobi_eigh(Msafe)
        ok = finite & (lam > 0).all(1) & np.isfinite(lam).all(1)
        s = 1.0 / np.sqrt(np.where(ok[:, None], lam, 1.0))
        W = np.einsum("nik,nk,njk->nij", V, s, V)
    return W, ok


def pair_terms(src, src_cov, tgt, tgt_cov, corr, R=None, kernel=(L2, 1.0, 1.0),
               route="eigh"):
    """-> (terms {m,3,29} float64: a row of the 29-sum layout per pair and
    Jacobian row, [28] = 1 in row 0 of a pair; ok {m}). A pair that cannot be
    whitened has zero terms."""
    corr = np.asarray(corr, np.int64).reshape(-1)
    sel = corr != -1
    c = corr[sel]
    vs = np.asarray(src, np.float64)[sel]
    vt = np.asarray(tgt, np.float64)[c]
    W, ok = whiten(np.asarray(src_cov)[sel], np.asarray(tgt_cov)[c], R, route)
    m = c.shape[0]
    d = vs - vt
    B = np.zeros((m, 3, 6))     # [-[vs]x | I]
    B[:, 0, 1], B[:, 0, 2] = vs[:, 2], -vs[:, 1]
    B[:, 1, 0], B[:, 1, 2] = -vs[:, 2], vs[:, 0]
    B[:, 2, 0], B[:, 2, 1] = vs[:, 1], -vs[:, 0]
    B[:, 0, 3] = B[:, 1, 4] = B[:, 2, 5] = 1.0
    J = W @ B                                   # {m,3,6}
    r = np.einsum("nij,nj->ni", W, d)           # {m,3}
    w = robust_weight(kernel, r)
    A = np.zeros((m, 3, 29))
    with np.errstate(all="ignore"):
        i = 0
        for j in range(6):
            for k in range(j + 1):
                A[:, :, i] = J[:, :, j] * w * J[:, :, k]
                i += 1
            A[:, :, 21 + j] = J[:, :, j] * w * r
        A[:, :, 27] = r * r
    A[:, 0, 28] = 1
    A[~ok] = 0
    return A, ok


def accumulate(*args, **kw):
    """-> (sums {32}: [0..28] the sums, [29] the pairs that could not be
    whitened, [30] = [31] = 0; abs_sums {29}: the sum of |term| per entry)."""
    A, ok = pair_terms(*args, **kw)
    sums = np.zeros(32)
    sums[:29] = A.sum((0, 1))
    sums[29] = (~ok).sum()
    return sums, np.abs(A).sum((0, 1))


def compute_rmse(src, src_cov, tgt, tgt_cov, corr):
    """sqrt(sum d^T W d / count), W = (Ct + Cs)^-1/2 -- W, not W^2: the
    reference's definition. No correspondence: 0. A pair that cannot be
    whitened adds 0 and stays in the count."""
    corr = np.asarray(corr, np.int64).reshape(-1)
    sel = corr != -1
    if not sel.any():
        return 0.0
    c = corr[sel]
    d = np.asarray(src, np.float64)[sel] - np.asarray(tgt, np.float64)[c]
    W, ok = whiten(np.asarray(src_cov)[sel], np.asarray(tgt_cov)[c])
    e = np.einsum("ni,nij,nj->n", d, W, d)
    return float(np.sqrt(e[ok].sum() / c.shape[0]))


def estimate_normals_knn(points, knn=20):
    """PointCloud::EstimateNormals(max_nn = knn) -- KNN search. The
    neighbourhood covariances are the reference's in the point dtype; the
    eigenvector is taken in float64 and narrowed, as everything here and as the
    library's EstimateNormals does for both dtypes (eigen3.h: the reference's
    Float32 eigen solver is good to about 1e-4 rad, which a 1e-6 rad pose
    parity cannot carry)."""
    idx, _ = orc.knn_search(points, points, knn)
    cnt = np.full(points.shape[0], idx.shape[1], np.int32)
    cov = orc.estimate_covariances(points, idx, cnt)
    nrm = orc.normals_from_covariances(cov.astype(np.float64))
    # An eigenvector has no sign, the reference's EstimateNormals leaves it to
    # its solver, and the covariance of a normal DOES depend on it inside the
    # cap e1 . n < -0.99 (covariances_from_normals). The library's
    # EstimateNormals pins it (eigen3.h): the last non-zero component is
    # positive.
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    flip = (z < 0) | ((z == 0) & ((y < 0) | ((y == 0) & (x < 0))))
    nrm[flip] *= -1.0
    return nrm.astype(points.dtype)


def initialize_covariances(points, covariances=None, normals=None,
                           epsilon=1e-3):
    """InitializePointCloudForGeneralizedICP: covariances given -> as they
    are; else from the normals; else from EstimateNormals(KNN 20)."""
    if covariances is not None:
        return np.asarray(covariances, points.dtype)
    if normals is None:
        normals = estimate_normals_knn(points, 20)
    return covariances_from_normals(np.asarray(normals, points.dtype), epsilon)


def _registration_result(source, target, max_dist):
    """ComputeRegistrationResult (Registration.cpp:24-62)."""
    idx, dist, cnt = orc.hybrid_search(target, source, max_dist, 1)
    corr = np.where(cnt > 0, idx[:, 0], -1).astype(np.int64)
    num = int((corr >= 0).sum())
    if num == 0:
        return corr, 0.0, 0.0
    sq = float(dist[:, 0][corr >= 0].astype(np.float64).sum())
    return corr, num / float(source.shape[0]), np.sqrt(sq / num)


def pyramid_level(pos, cov, voxel_size):
    """PointCloud::VoxelDownSample of positions and covariances: the nine
    columns averaged like any attribute, as three {n,3} row tables."""
    rows = []
    down = None
    for r in range(3):
        down, o = orc.voxel_down_sample(
            pos, np.ascontiguousarray(cov[:, r, :]), voxel_size)
        rows.append(o)
    return down, np.ascontiguousarray(np.stack(rows, 1))


def multiscale_icp(source, target, voxel_sizes, criterias, max_dists,
                   init=None, source_covariances=None, target_covariances=None,
                   source_normals=None, target_normals=None, epsilon=1e-3,
                   kernel=(L2, 1.0, 1.0), rotate_covariances=True):
    """MultiScaleICP (Registration.cpp:362-444) with the generalized
    estimator. criterias: (relative_fitness, relative_rmse, max_iteration) per
    scale. The level's source positions stand at the cumulative
    transformation; its covariances stay as built and are rotated per pair by
    the rotation of that transformation (rotate_covariances=False: left as
    they are -- the mistake the tests must be able to tell). -> dict with
    transformation, fitness, inlier_rmse, converged, num_iterations,
    level_sizes [(ns, nt)], singular_pairs (of the last accumulate)."""
    dt = source.dtype
    S = len(criterias)
    s_cur = (source, initialize_covariances(source, source_covariances,
                                            source_normals, epsilon))
    t_cur = (np.asarray(target, dt),
             initialize_covariances(np.asarray(target, dt), target_covariances,
                                    target_normals, epsilon))
    src_levels, tgt_levels = [None] * S, [None] * S
    for k in range(S - 1, -1, -1):
        if voxel_sizes[k] > 0:
            s_cur = pyramid_level(s_cur[0], s_cur[1], voxel_sizes[k])
            t_cur = pyramid_level(t_cur[0], t_cur[1], voxel_sizes[k])
        src_levels[k], tgt_levels[k] = s_cur, t_cur
    T = np.array(np.eye(4) if init is None else init, np.float64)
    fitness = rmse = 0.0
    converged = False
    total = 0
    singular = 0
    for k in range(S):
        pos, cov = src_levels[k]
        tpos, tcov = tgt_levels[k]
        pos = orc.transform_points(T, pos)
        prev_fitness, prev_rmse = fitness, rmse
        converged = False
        rf, rr, max_it = criterias[k]
        it = 0
        while it < max_it:
            corr, fitness, rmse = _registration_result(pos, tpos, max_dists[k])
            if not (corr >= 0).any():
                T = np.eye(4)
            if fitness <= np.finfo(np.float64).tiny:
                break
            sums, _ = accumulate(pos, cov, tpos, tcov, corr,
                                 T[:3, :3] if rotate_covariances else None,
                                 kernel)
            singular = int(sums[29])
            st, pose, _, _ = orc.decode_and_solve6x6(sums[:29])
            if st != 0:
                raise RuntimeError("Singular 6x6 linear system detected")
            update = orc.pose_to_transformation(pose)
            T = update @ T
            pos = orc.transform_points(update, pos)
            if (it != 0 and abs(prev_fitness - fitness) < rf and
                    abs(prev_rmse - rmse) < rr):
                converged = True
                break
            prev_fitness, prev_rmse = fitness, rmse
            it += 1
        total += it
        if k == S - 1:
            corr, fitness, rmse = _registration_result(pos, tpos, max_dists[k])
            if not (corr >= 0).any():
                T = np.eye(4)
        if fitness <= np.finfo(np.float64).tiny:
            converged = False
            break
    return dict(transformation=T, fitness=fitness, inlier_rmse=rmse,
                converged=converged, num_iterations=total,
                level_sizes=[(src_levels[k][0].shape[0],
                              tgt_levels[k][0].shape[0]) for k in range(S)],
                singular_pairs=singular)


# ---- the accumulate cases shared by the CPU and the GPU tests ---------------
SIZES = (1, 63, 64, 65, 257, 4099)
SETTINGS = {
    "l2": (L2, 1.0, 1.0),
    "huber": (HUBER, 0.03, 1.0),
    "tukey": (TUKEY, 0.05, 1.0),
    "cauchy": (CAUCHY, 0.05, 1.0),
}
R_SOURCE = None


def r_source():
    """A non-identity rotation the source positions are taken to have
    received."""
    global R_SOURCE
    if R_SOURCE is None:
        R_SOURCE = np.ascontiguousarray(orc.pose_to_transformation(
            [0.3, -0.2, 0.5, 0, 0, 0])[:3, :3])
    return R_SOURCE


def accumulate_case(n, dtype, seed=0):
    """n source rows against 3 n / 4 + 5 target points, ~20 % of rows -1, the
    pairs a few centimetres apart; covariances from noisy unit normals at
    epsilon = 1e-3 (the source's in the frame before r_source()).
    -> ([src, src_cov, tgt, tgt_cov, corr], nt)."""
    rng = np.random.default_rng(seed + n)
    nt = 3 * n // 4 + 5
    tgt = rng.uniform(-3, 3, (nt, 3))
    tn = rng.standard_normal((nt, 3))
    tn /= np.linalg.norm(tn, axis=1, keepdims=True)
    corr = rng.integers(0, nt, n).astype(np.int64)
    src = tgt[corr] + 0.05 * rng.standard_normal((n, 3))
    sn = tn[corr] + 0.1 * rng.standard_normal((n, 3))
    sn /= np.linalg.norm(sn, axis=1, keepdims=True)
    sn = sn @ r_source()            # R^T n: the normal before the rotation
    corr[rng.random(n) < 0.2] = -1
    if n == 1:
        corr[0] = nt - 1
    src, sn, tgt, tn = (np.ascontiguousarray(a.astype(dtype))
                        for a in (src, sn, tgt, tn))
    return [src, covariances_from_normals(sn, 1e-3), tgt,
            covariances_from_normals(tn, 1e-3), corr], nt
