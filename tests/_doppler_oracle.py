"""numpy restatement of TransformationEstimationForDopplerICP (Hexsel et al.,
"DICP: Doppler Iterative Closest Point Algorithm", RSS 2022) as the reference
computes it, for the Doppler ICP tests.

  transformation_to_pose   TransformationToPoseImpl (kernel/
                           TransformationConverterImpl.h:44-60)
  host_prepare             ComputePoseDopplerICP up to its per-device call
                           (kernel/Registration.cpp:222-265)
  accumulate               GetJacobianDopplerICP + the 29 sums of
                           ComputePoseDopplerICPKernelCPU (RegistrationImpl.h:
                           525-643, RegistrationCPU.cpp:336-493)
  multiscale_icp           DoSingleScaleICPIterations / MultiScaleICP
                           (Registration.cpp:275-444) with this estimator

Per-pair terms are formed in the point dtype, one numpy operation per
operation of the reference (numpy rounds every operation to the array's dtype
and fuses nothing); the 29 sums are float64. Search, VoxelDownSample, the 6x6
solve and the pose/transform helpers are _oracle's.
"""
import numpy as np

import _oracle as orc

L2, L1, HUBER, CAUCHY, GM, TUKEY, GENERALIZED = range(7)

DEFAULTS = dict(period=0.1, lambda_doppler=0.01, reject_dynamic_outliers=False,
                doppler_outlier_threshold=2.0,
                outlier_rejection_min_iteration=2,
                geometric_robust_loss_min_iteration=0,
                doppler_robust_loss_min_iteration=2,
                geometric_kernel=(L2, 1.0, 1.0), doppler_kernel=(L2, 1.0, 1.0),
                transform_vehicle_to_sensor=None)


def transformation_to_pose(T):
    T = np.asarray(T, np.float64).reshape(16)
    sy = np.sqrt(T[0] * T[0] + T[4] * T[4])
    pose = np.zeros(6, np.float64)
    if not (sy < 1e-6):
        pose[0] = np.arctan2(T[9], T[10])
        pose[1] = np.arctan2(-T[8], sy)
        pose[2] = np.arctan2(T[4], T[0])
    else:
        pose[0] = np.arctan2(-T[6], T[5])
        pose[1] = np.arctan2(-T[8], sy)
        pose[2] = 0
    pose[3:] = T[[3, 7, 11]]
    return pose


def robust_weight(kernel, r):
    """RobustKernelImpl.h:35-126 on an array of residuals of the point dtype:
    the double-typed literals promote parts of each expression to float64
    before the result is narrowed."""
    method, scaling, shape = kernel
    dt = r.dtype.type
    scale = dt(scaling)
    f64 = np.float64
    if method == L2:
        return np.ones_like(r)
    if method == L1:
        with np.errstate(divide="ignore"):
            return (1.0 / np.abs(r).astype(f64)).astype(dt)
    if method == HUBER:
        a = np.abs(r)
        return scale / np.where(a < scale, scale, a)
    if method == CAUCHY:
        q = r / scale
        return (1.0 / (1.0 + (q * q).astype(f64))).astype(dt)
    if method == GM:
        s = scale + r * r
        return scale / (s * s)
    if method == TUKEY:
        a = np.abs(r) / scale
        m = np.where(dt(1.0) < a, dt(1.0), a)
        v = 1.0 - (m * m).astype(f64)
        return (v * v).astype(dt)
    return np.array([orc.robust_weight(method, scaling, shape, float(x),
                                       f64=r.dtype == np.float64)
                     for x in r], dtype=r.dtype)


def reference_accepts(method_geometric, method_doppler):
    """DISPATCH_DUAL_ROBUST_KERNEL_FUNCTION (RobustKernelImpl.h:122-179), the
    dispatch of ComputePoseDopplerICP{CPU,CUDA}, has branches for L2Loss and
    TukeyLoss only and takes no shape parameter: any other pair of kernels,
    GeneralizedLoss included, is "Unsupported method." in the reference. The
    library (and robust_weight above) weighs each term with the single-kernel
    dispatch instead, which gives the same bits on the four pairs the
    reference runs."""
    return (method_geometric in (L2, TUKEY)) and (method_doppler in (L2, TUKEY))


def kernels_at(iteration, p):
    """The kernels and the rejection in force at `iteration` of a scale."""
    default = (L2, 1.0, 1.0)
    kg = (p["geometric_kernel"]
          if iteration >= p["geometric_robust_loss_min_iteration"] else default)
    kd = (p["doppler_kernel"]
          if iteration >= p["doppler_robust_loss_min_iteration"] else default)
    reject = bool(p["reject_dynamic_outliers"] and
                  iteration >= p["outlier_rejection_min_iteration"])
    return kg, kd, reject


def host_prepare(transform_vehicle_to_sensor, current_transform, period, dtype):
    """-> R_S_to_V {9}, r_v_to_s_in_V {3}, w_v_in_V {3}, v_v_in_V {3}, all of
    the point dtype."""
    dt = np.dtype(dtype).type
    V = np.asarray(np.eye(4) if transform_vehicle_to_sensor is None
                   else transform_vehicle_to_sensor, np.float64)
    R = np.linalg.inv(V[:3, :3]).reshape(9).astype(dt)
    r = V[:3, 3].astype(dt)
    state = transformation_to_pose(current_transform).astype(dt)
    # Tensor::Div(Scalar): the scalar is cast to the tensor's dtype first
    w = (-state[:3]) / dt(period)
    v = (-state[3:]) / dt(period)
    return R, r, w, v


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2],
            a[0] * b[1] - a[1] * b[0]]


def _matvec(R, x):
    return [R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2]
            for i in range(3)]


def predicted_doppler(directions, R, r, w, v):
    """-dot(R_S_to_V d, v_s_in_S) per point, in the point dtype: the
    reference's own prediction (RegistrationImpl.h:525-541,589-593)."""
    v_s_in_V = _cross(w, r)
    v_s_in_V = [v_s_in_V[k] + v[k] for k in range(3)]
    v_s_in_S = _matvec(R, v_s_in_V)
    d = [directions[:, k] for k in range(3)]
    ds_in_S = _matvec(R, d)
    return -(ds_in_S[0] * v_s_in_S[0] + ds_in_S[1] * v_s_in_S[1] +
             ds_in_S[2] * v_s_in_S[2])


def pair_terms(src, dopplers, directions, tgt, tgt_n, corr, R, r, w, v,
               period, reject, threshold, kernel_geometric, kernel_doppler,
               lambda_doppler):
    """-> (terms {m,29} of the point dtype for the m rows with a
    correspondence, rejected {m} bool)."""
    dt = src.dtype.type
    corr = np.asarray(corr, np.int64).reshape(-1)
    sel = corr != -1
    c = corr[sel]
    ps = [src[sel, k] for k in range(3)]
    ds = [directions[sel, k] for k in range(3)]
    pt = [tgt[c, k] for k in range(3)]
    nt = [tgt_n[c, k] for k in range(3)]
    doppler_in_S = np.asarray(dopplers).reshape(-1)[sel]
    R, r, w, v = (np.asarray(a, src.dtype) for a in (R, r, w, v))
    slg = dt(np.sqrt(1.0 - np.float64(dt(lambda_doppler))))
    sld = dt(np.sqrt(np.float64(lambda_doppler)))
    sld_dt = sld / dt(period)
    pred = predicted_doppler(np.stack(ds, 1), R, r, w, v)
    doppler_error = (doppler_in_S - pred).astype(np.float64)
    rejected = (np.abs(doppler_error) > np.float64(dt(threshold))
                if reject else np.zeros(c.shape, bool))
    J_D_w = _cross(ds, r)
    J_D = [sld_dt * J_D_w[0], sld_dt * J_D_w[1], sld_dt * J_D_w[2],
           sld_dt * -ds[0], sld_dt * -ds[1], sld_dt * -ds[2]]
    r_D = (np.float64(sld) * doppler_error).astype(dt)
    p2p = ((ps[0] - pt[0]) * nt[0] + (ps[1] - pt[1]) * nt[1] +
           (ps[2] - pt[2]) * nt[2])
    J_G = [slg * (-ps[2] * nt[1] + ps[1] * nt[2]),
           slg * (ps[2] * nt[0] - ps[0] * nt[2]),
           slg * (-ps[1] * nt[0] + ps[0] * nt[1]),
           slg * nt[0], slg * nt[1], slg * nt[2]]
    r_G = slg * p2p
    with np.errstate(all="ignore"):
        w_G = robust_weight(kernel_geometric, r_G)
        w_D = robust_weight(kernel_doppler, r_D)
        A = np.zeros((c.shape[0], 29), src.dtype)
        i = 0
        for j in range(6):
            for k in range(j + 1):
                A[:, i] = J_G[j] * w_G * J_G[k] + J_D[j] * w_D * J_D[k]
                i += 1
            A[:, 21 + j] = J_G[j] * w_G * r_G + J_D[j] * w_D * r_D
        A[:, 27] = r_G * r_G + r_D * r_D
    A[:, 28] = 1
    # a rejected pair: Jacobians and residuals stay zero, the count is kept
    A[rejected, :28] = 0
    return A, rejected


def accumulate(*args, **kw):
    """The 29 float64 sums."""
    A, _ = pair_terms(*args, **kw)
    return A.astype(np.float64).sum(0)


def _registration_result(source, target, max_dist):
    """ComputeRegistrationResult (Registration.cpp:24-62)."""
    idx, dist, cnt = orc.hybrid_search(target, source, max_dist, 1)
    corr = np.where(cnt > 0, idx[:, 0], -1).astype(np.int64)
    num = int((corr >= 0).sum())
    if num == 0:
        return corr, 0.0, 0.0
    sq = float(dist[:, 0][corr >= 0].astype(np.float64).sum())
    return corr, num / float(source.shape[0]), np.sqrt(sq / num)


def _pad(col):
    """{n,1} as column 0 of {n,3}: _oracle's VoxelDownSample takes {n,3}
    attributes and averages every column on its own."""
    out = np.zeros((col.shape[0], 3), col.dtype)
    out[:, 0] = col.reshape(-1)
    return out


def pyramid_level(pos, attrs, voxel_size):
    """PointCloud::VoxelDownSample of positions and {n,3} attributes (voxels in
    first-occurrence order, every attribute averaged)."""
    outs = []
    down = None
    for a in attrs:
        down, o = orc.voxel_down_sample(pos, a, voxel_size)
        outs.append(o)
    if not attrs:
        down, _ = orc.voxel_down_sample(pos, None, voxel_size)
    return down, outs


def multiscale_icp(source, dopplers, directions, target, target_normals,
                   voxel_sizes, criterias, max_dists, init=None, params=None,
                   estimation="doppler"):
    """MultiScaleICP (Registration.cpp:362-444). criterias: (relative_fitness,
    relative_rmse, max_iteration) per scale. estimation "plane": the same
    driver with point-to-plane L2 updates (no Doppler term) on the same
    clouds. -> dict with transformation, fitness, inlier_rmse, converged,
    num_iterations, level_sizes [(ns, nt)], kernels_used [[(kg, kd, reject)]]
    per scale and iteration."""
    p = dict(DEFAULTS)
    p.update(params or {})
    if not (0.0 <= p["lambda_doppler"] <= 1.0):
        p["lambda_doppler"] = 0.01
    dt = source.dtype
    S = len(criterias)
    # InitializePointCloudPyramidForMultiScaleICP :221-273
    src_levels, tgt_levels = [None] * S, [None] * S
    s_cur = (source, _pad(np.asarray(dopplers, dt)), np.asarray(directions, dt))
    t_cur = (np.asarray(target, dt), np.asarray(target_normals, dt))
    for k in range(S - 1, -1, -1):
        if voxel_sizes[k] > 0:
            pos, (dop3, dirs) = pyramid_level(s_cur[0], [s_cur[1], s_cur[2]],
                                              voxel_sizes[k])
            s_cur = (pos, dop3, dirs)
            tpos, (tn,) = pyramid_level(t_cur[0], [t_cur[1]], voxel_sizes[k])
            t_cur = (tpos, tn)
        src_levels[k], tgt_levels[k] = s_cur, t_cur
    T = np.array(np.eye(4) if init is None else init, np.float64)
    fitness = rmse = 0.0
    converged = False
    total = 0
    used = []
    for k in range(S):
        pos, dop3, dirs = src_levels[k]
        tpos, tn = tgt_levels[k]
        pos = orc.transform_points(T, pos)      # directions are NOT rotated
        dop = np.ascontiguousarray(dop3[:, 0])
        prev_fitness, prev_rmse = fitness, rmse
        converged = False
        rf, rr, max_it = criterias[k]
        used.append([])
        it = 0
        while it < max_it:
            corr, fitness, rmse = _registration_result(pos, tpos, max_dists[k])
            if not (corr >= 0).any():
                T = np.eye(4)
            if fitness <= np.finfo(np.float64).tiny:
                break
            if estimation == "doppler":
                kg, kd, reject = kernels_at(it, p)
                used[-1].append((kg, kd, reject))
                R, r, w, v = host_prepare(p["transform_vehicle_to_sensor"], T,
                                          p["period"], dt)
                sums = accumulate(pos, dop, dirs, tpos, tn, corr, R, r, w, v,
                                  p["period"], reject,
                                  p["doppler_outlier_threshold"], kg, kd,
                                  p["lambda_doppler"])
            else:
                sums = orc.p2plane_accumulate(pos, tpos, tn, corr,
                                              accumulate_double=True)
            st, pose, _, _ = orc.decode_and_solve6x6(sums)
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
                kernels_used=used)


def doppler_at(directions, transformation, params=None):
    """Dopplers of a static scene for source -> target motion `transformation`
    over one period: the reference's own prediction at that motion, so the
    Doppler residual is zero there."""
    p = dict(DEFAULTS)
    p.update(params or {})
    R, r, w, v = host_prepare(p["transform_vehicle_to_sensor"], transformation,
                              p["period"], directions.dtype)
    return predicted_doppler(directions, R, r, w, v)


def plane_scene(n=5000, seed=5, dtype=np.float64, motion=(0.30, 0.10)):
    """The case the estimator exists for: a single (ground) plane 1.5 m under
    the sensor, sampled independently in the two scans, the sensor translating
    INSIDE the plane by `motion` between them. Geometry says nothing about that
    translation; the Doppler velocities do. 1 cm of range noise and slightly
    noisy target normals keep the 6x6 systems non-singular."""
    rng = np.random.default_rng(seed)
    T_gt = np.eye(4)
    T_gt[0, 3], T_gt[1, 3] = motion

    def scan():
        p = np.empty((n, 3))
        p[:, :2] = rng.uniform(-8.0, 8.0, (n, 2))
        p[:, 2] = -1.5 + 0.01 * rng.standard_normal(n)
        return p
    source, target = scan(), scan()
    nrm = np.array([0.0, 0.0, 1.0]) + 0.02 * rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    source = source.astype(dtype)
    directions = (source / np.linalg.norm(source, axis=1, keepdims=True))
    dopplers = doppler_at(directions, T_gt)
    return dict(source=source, target=target.astype(dtype),
                target_normals=nrm.astype(dtype), directions=directions,
                dopplers=dopplers, T_gt=T_gt, max_dist=1.0,
                criteria=(1e-6, 1e-6, 30))


def in_plane_error(T, T_gt):
    return float(np.hypot(T[0, 3] - T_gt[0, 3], T[1, 3] - T_gt[1, 3]))
