"""Python mirror of open3d.t.pipelines.registration.{icp, multi_scale_icp,
compute_fpfh_feature, correspondences_from_features} for the MI355X backend
(point-to-plane and point-to-point estimators), and of the legacy
open3d.pipelines.registration.registration_ransac_based_on_{correspondence,
feature_matching} with their correspondence checkers.

Argument names / defaults follow the reference's binding
(cpp/pybind/t/pipelines/registration/registration.cpp) and
t/pipelines/registration/Registration.h:31-98,133-208. Point clouds are given
as torch device tensors {N,3} (float32 or float64).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .core import TORCH_TO_O3DMI, require_cuda, stream


class ICPConvergenceCriteria:
    def __init__(self, relative_fitness=1e-6, relative_rmse=1e-6,
                 max_iteration=30):
        self.relative_fitness = relative_fitness
        self.relative_rmse = relative_rmse
        self.max_iteration = max_iteration


class RobustKernel:
    L2Loss, L1Loss, HuberLoss, CauchyLoss, GMLoss, TukeyLoss, \
        GeneralizedLoss = range(7)

    def __init__(self, type=0, scaling_parameter=1.0, shape_parameter=1.0):
        self.type = type
        self.scaling_parameter = scaling_parameter
        self.shape_parameter = shape_parameter


class TransformationEstimationPointToPlane:
    def __init__(self, kernel=None):
        self.kernel = kernel or RobustKernel()


class TransformationEstimationPointToPoint:
    """TransformationEstimation.h:76-118; no robust kernel, no normals.
    with_scaling (the legacy estimator's argument) is read by the RANSAC
    functions only, which reject it."""
    kernel = RobustKernel()

    def __init__(self, with_scaling=False):
        self.with_scaling = with_scaling


class TransformationEstimationSymmetric:
    """TransformationEstimation.h (Symmetric ICP, Rusinkiewicz 2019): needs
    source and target normals."""
    def __init__(self, kernel=None):
        self.kernel = kernel or RobustKernel()


class TransformationEstimationForColoredICP:
    """TransformationEstimation.h:283-349 (Park et al. 2017): needs target
    normals and colours on both clouds; `color_gradients` of the target are
    estimated when not given."""
    def __init__(self, lambda_geometric=0.968, kernel=None):
        self.lambda_geometric = lambda_geometric
        self.kernel = kernel or RobustKernel()


class TransformationEstimationForDopplerICP:
    """TransformationEstimation.h:356-500 (Hexsel et al., DICP, RSS 2022):
    needs target normals and, on the source, `dopplers` {N,1} and `directions`
    {N,3} (unit vectors of the vehicle frame, compute_direction_vectors).
    The robust kernels and the dynamic-outlier rejection switch on at the
    given iteration indices, which restart at 0 at every scale."""
    def __init__(self, period=0.1, lambda_doppler=0.01,
                 reject_dynamic_outliers=False, doppler_outlier_threshold=2.0,
                 outlier_rejection_min_iteration=2,
                 geometric_robust_loss_min_iteration=0,
                 doppler_robust_loss_min_iteration=2, geometric_kernel=None,
                 doppler_kernel=None, transform_vehicle_to_sensor=None):
        self.period = period
        # TransformationEstimation.h:389-391
        self.lambda_doppler = (lambda_doppler
                               if 0.0 <= lambda_doppler <= 1.0 else 0.01)
        self.reject_dynamic_outliers = reject_dynamic_outliers
        self.doppler_outlier_threshold = doppler_outlier_threshold
        self.outlier_rejection_min_iteration = outlier_rejection_min_iteration
        self.geometric_robust_loss_min_iteration = \
            geometric_robust_loss_min_iteration
        self.doppler_robust_loss_min_iteration = \
            doppler_robust_loss_min_iteration
        self.geometric_kernel = geometric_kernel or RobustKernel()
        self.doppler_kernel = doppler_kernel or RobustKernel()
        self.transform_vehicle_to_sensor = np.array(
            np.eye(4) if transform_vehicle_to_sensor is None
            else transform_vehicle_to_sensor, dtype=np.float64)
        if self.transform_vehicle_to_sensor.shape != (4, 4):
            raise ValueError("transform_vehicle_to_sensor must be 4x4")
    kernel = RobustKernel()

    def _fill(self, d):
        """-> the o3dmi_icp_doppler_t fields that are not pointers."""
        d.transform_vehicle_to_sensor[:] = \
            self.transform_vehicle_to_sensor.reshape(-1).tolist()
        d.period = self.period
        d.lambda_doppler = self.lambda_doppler
        d.reject_dynamic_outliers = 1 if self.reject_dynamic_outliers else 0
        d.doppler_outlier_threshold = self.doppler_outlier_threshold
        d.outlier_rejection_min_iteration = \
            int(self.outlier_rejection_min_iteration)
        d.geometric_robust_loss_min_iteration = \
            int(self.geometric_robust_loss_min_iteration)
        d.doppler_robust_loss_min_iteration = \
            int(self.doppler_robust_loss_min_iteration)
        d.geometric_kernel = int(self.geometric_kernel.type)
        d.geometric_scaling_parameter = self.geometric_kernel.scaling_parameter
        d.geometric_shape_parameter = self.geometric_kernel.shape_parameter
        d.doppler_kernel = int(self.doppler_kernel.type)
        d.doppler_scaling_parameter = self.doppler_kernel.scaling_parameter
        d.doppler_shape_parameter = self.doppler_kernel.shape_parameter


class TransformationEstimationForGeneralizedICP:
    """Legacy pipelines/registration/GeneralizedICP.h (Segal et al.,
    "Generalized-ICP", RSS 2009): reads a covariance {N,3,3} per point of both
    clouds. A cloud without `covariances` gets them from its normals
    (covariances_from_normals with `epsilon`), one without normals from
    EstimateNormals with KNN 20 first."""
    def __init__(self, epsilon=1e-3, kernel=None):
        self.epsilon = epsilon
        self.kernel = kernel or RobustKernel()


def covariances_from_normals(normals, epsilon=1e-3):
    """InitializePointCloudForGeneralizedICP's covariances {N,3,3} from
    normals {N,3}: Rx diag(epsilon,1,1) Rx^T with Rx the rotation from e1 to
    the normal (GeneralizedICP.cpp:33-80)."""
    normals = require_cuda(normals, "normals")
    if normals.dtype not in (torch.float32, torch.float64):
        raise ValueError("Only Float32 and Float64 point clouds are supported.")
    if normals.dim() != 2 or normals.shape[1] != 3:
        raise ValueError("normals must be {N,3}")
    out = torch.empty((normals.shape[0], 3, 3), dtype=normals.dtype,
                      device=normals.device)
    _lib.check(_lib.lib().o3dmi_pointcloud_covariances_from_normals(
        _lib.ptr(normals), normals.shape[0], TORCH_TO_O3DMI[normals.dtype],
        C.c_double(epsilon), _lib.ptr(out), stream()),
        "covariances_from_normals")
    return out


def _covariances(t, name, like):
    t = require_cuda(t, name)
    if t.dtype != like.dtype:
        raise ValueError("source / attribute dtype mismatch")
    if tuple(t.shape) != (like.shape[0], 3, 3):
        raise ValueError(name + " must be {N,3,3}")
    return t


def transformation_to_pose(transformation):
    """t::pipelines::kernel::TransformationToPose: 4x4 -> pose {6} (Euler
    angles, translation), float64."""
    T = np.ascontiguousarray(transformation, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("transformation must be 4x4")
    pose = np.zeros(6, np.float64)
    _lib.lib().o3dmi_transformation_to_pose(_lib.f64p(T), _lib.f64p(pose))
    return pose


def compute_direction_vectors(positions):
    """Unit direction of every point seen from the origin, p / |p| (the helper
    of the reference's Doppler ICP tests and examples); torch or numpy."""
    if isinstance(positions, torch.Tensor):
        return positions / torch.linalg.norm(positions, dim=1, keepdim=True)
    positions = np.asarray(positions)
    return positions / np.linalg.norm(positions, axis=1, keepdims=True)


class RegistrationResult:
    def __init__(self):
        self.transformation = np.eye(4)
        self.correspondence_set = None
        self.inlier_rmse = 0.0
        self.fitness = 0.0
        self.converged = False
        self.num_iterations = 0


def multi_scale_icp(source, target, target_normals, voxel_sizes, criteria_list,
                    max_correspondence_distances, init_source_to_target=None,
                    estimation_method=None, callback_after_iteration=None,
                    allreduce=None, source_normals=None, source_colors=None,
                    target_colors=None, target_color_gradients=None,
                    device_allreduce=None, device_counts=None,
                    level_sharding=False, source_dopplers=None,
                    source_directions=None, source_covariances=None,
                    target_covariances=None, return_singular_pairs=False):
    """source/target/target_normals: device tensors {N,3}. `device_counts`
    (optional): (ns, nt) int32 device tensors of one element holding the LIVE
    sizes of source / target, whose tensors are then buffers of at least that
    many rows (o3dmi_icp_options_t: no read-back of the sizes). `allreduce`
    (optional) sums a length-32 numpy float64 array over ranks in place;
    `device_allreduce(dev_ptr, n, stream_ptr)` (optional, takes precedence;
    sharding.make_device_allreduce) enqueues the same sum on the device.
    `level_sharding`: with a communicator installed (sharding.Comm.install)
    every rank passes the WHOLE source and the driver shards each pyramid
    level; otherwise each rank passes its shard.
    `source_normals` is read by the symmetric estimator, the colours (and the
    optional target colour gradients) by the coloured one, `source_dopplers`
    {N,1} (or {N}) and `source_directions` {N,3} by the Doppler one. The
    generalized estimator reads `source_covariances` / `target_covariances`
    {N,3,3}; for a cloud without them `source_normals` / `target_normals`,
    which may both be None for it. `return_singular_pairs` (generalized only):
    returns (result, the pairs of the last iteration that could not be
    whitened)."""
    est = estimation_method or TransformationEstimationPointToPlane()
    generalized = isinstance(est, TransformationEstimationForGeneralizedICP)
    if return_singular_pairs and not generalized:
        raise ValueError("return_singular_pairs is of the generalized "
                         "estimator")
    gen = _lib.IcpGeneralized()
    singular_pairs = C.c_int64(0)
    gen_source_normals = source_normals if generalized else None
    doppler = isinstance(est, TransformationEstimationForDopplerICP)
    dop = _lib.IcpDoppler()
    if doppler:
        if target_normals is None:
            raise ValueError("DopplerICP requires target pointcloud to have "
                             "normals.")
        if source_dopplers is None:
            raise ValueError("DopplerICP requires source pointcloud to have "
                             "Doppler velocities.")
        if source_directions is None:
            raise ValueError("DopplerICP requires source pointcloud to have "
                             "pre-computed direction vectors.")
        source_dopplers = require_cuda(source_dopplers, "source_dopplers")
        source_directions = require_cuda(source_directions,
                                         "source_directions")
        est._fill(dop)
        dop.source_dopplers = source_dopplers.data_ptr()
        dop.source_directions = source_directions.data_ptr()
    p2point = isinstance(est, TransformationEstimationPointToPoint)
    symmetric = isinstance(est, TransformationEstimationSymmetric)
    if symmetric:
        if source_normals is None or target_normals is None:
            raise ValueError("SymmetricICP requires both source and target to "
                             "have normals.")
        source_normals = require_cuda(source_normals, "source_normals")
    else:
        source_normals = None
    colored = isinstance(est, TransformationEstimationForColoredICP)
    attrs = _lib.IcpAttributes()
    attrs.lambda_geometric = getattr(est, "lambda_geometric", 0.968)
    if colored:
        if source_colors is None or target_colors is None:
            raise ValueError("Source and/or Target pointcloud missing colors "
                             "attribute.")
        source_colors = require_cuda(source_colors, "source_colors")
        target_colors = require_cuda(target_colors, "target_colors")
        attrs.source_colors = source_colors.data_ptr()
        attrs.target_colors = target_colors.data_ptr()
        if target_color_gradients is not None:
            target_color_gradients = require_cuda(target_color_gradients,
                                                  "target_color_gradients")
            attrs.target_color_gradients = target_color_gradients.data_ptr()
    if symmetric:
        attrs.source_normals = source_normals.data_ptr()
    source = require_cuda(source, "source")
    target = require_cuda(target, "target")
    if source.dtype not in (torch.float32, torch.float64):
        raise ValueError("Only Float32 and Float64 point clouds are supported.")
    if target.dtype != source.dtype:
        raise ValueError("source / target dtype mismatch")
    if doppler:
        if (source_dopplers.dtype != source.dtype or
                source_directions.dtype != source.dtype):
            raise ValueError("source / attribute dtype mismatch")
        if (source_dopplers.numel() != source.shape[0] or
                tuple(source_directions.shape) != tuple(source.shape)):
            raise ValueError("dopplers must be {N,1} and directions {N,3}")
    if generalized:
        gen.epsilon = est.epsilon
        gen.robust_kernel = int(est.kernel.type)
        gen.scaling_parameter = est.kernel.scaling_parameter
        gen.shape_parameter = est.kernel.shape_parameter
        gen.singular_pairs_out = C.pointer(singular_pairs)
        if source_covariances is not None:
            source_covariances = _covariances(source_covariances,
                                              "source_covariances", source)
            gen.source_covariances = source_covariances.data_ptr()
        if target_covariances is not None:
            target_covariances = _covariances(target_covariances,
                                              "target_covariances", target)
            gen.target_covariances = target_covariances.data_ptr()
        if gen_source_normals is not None:
            gen_source_normals = require_cuda(gen_source_normals,
                                              "source_normals")
            if (gen_source_normals.dtype != source.dtype or
                    tuple(gen_source_normals.shape) != tuple(source.shape)):
                raise ValueError("source_normals must be {N,3} of the "
                                 "source's dtype")
            gen.source_normals = gen_source_normals.data_ptr()
    if p2point or (generalized and target_normals is None):
        target_normals = None
    else:
        if target_normals is None:
            raise ValueError("Target pointcloud missing normals attribute.")
        target_normals = require_cuda(target_normals, "target_normals")
        if target_normals.dtype != source.dtype:
            raise ValueError("source / target dtype mismatch")
    S = len(criteria_list)
    if not (len(voxel_sizes) == S and len(max_correspondence_distances) == S):
        raise ValueError("Size of criterias, voxel_size, "
                         "max_correspondence_distances vectors must be same.")
    vs = np.ascontiguousarray(voxel_sizes, dtype=np.float64)
    md = np.ascontiguousarray(max_correspondence_distances, dtype=np.float64)
    crit = (_lib.IcpCriteria * S)(*[
        _lib.IcpCriteria(c.relative_fitness, c.relative_rmse, c.max_iteration)
        for c in criteria_list])
    init = np.ascontiguousarray(
        np.eye(4) if init_source_to_target is None else init_source_to_target,
        dtype=np.float64)
    if init.shape != (4, 4):
        raise ValueError("init_source_to_target must be 4x4")
    ns, nt = source.shape[0], target.shape[0]
    corr = torch.full((ns,), -1, dtype=torch.int64, device="cuda")
    res = _lib.RegistrationResultC()

    cb = _lib.ICP_CALLBACK(0)
    if callback_after_iteration is not None:
        def _cb(it, sc, sit, rmse, fit, Tp, user):
            callback_after_iteration({
                "iteration_index": it, "scale_index": sc,
                "scale_iteration_index": sit, "inlier_rmse": rmse,
                "fitness": fit,
                "transformation": np.ctypeslib.as_array(
                    Tp, shape=(16,)).reshape(4, 4).copy()})
        cb = _lib.ICP_CALLBACK(_cb)
    ar = _lib.ALLREDUCE_SUM(0)
    if allreduce is not None:
        def _ar(buf, n, user):
            a = np.ctypeslib.as_array(buf, shape=(n,))
            allreduce(a)
            return 0
        ar = _lib.ALLREDUCE_SUM(_ar)

    opts = _lib.IcpOptions()
    opts.level_sharding = 1 if level_sharding else 0
    if device_counts is not None:
        ns_dev, nt_dev = device_counts
        opts.ns_dev = ns_dev.data_ptr()
        opts.nt_dev = nt_dev.data_ptr()
    if device_allreduce is not None:
        def _dar(buf, n, strm, user):
            try:
                device_allreduce(int(buf or 0), int(n), int(strm or 0))
                return 0
            except Exception:  # surfaces as the driver's error status
                import traceback
                traceback.print_exc()
                return 1
        # (`dar` keeps the callback object alive for the call)
        dar = _lib.ALLREDUCE_DEVICE(_dar)
        opts.device_allreduce = dar
    common = (_lib.ptr(source), ns, _lib.ptr(target),
              _lib.ptr(target_normals) if target_normals is not None else None,
              nt, TORCH_TO_O3DMI[source.dtype], S, _lib.f64p(vs), crit,
              _lib.f64p(md), _lib.f64p(init))
    tail = (cb, None, ar, None, _lib.ptr(corr), C.byref(res), stream())
    if doppler:
        st = _lib.lib().o3dmi_registration_multiscale_icp_doppler(
            *common, C.byref(dop), C.byref(opts), *tail)
    elif generalized:
        st = _lib.lib().o3dmi_registration_multiscale_icp_generalized(
            *common, C.byref(gen), C.byref(opts), *tail)
    else:
        st = _lib.lib().o3dmi_registration_multiscale_icp_ex(
            *common,
            1 if p2point else (2 if symmetric else (3 if colored else 0)),
            C.byref(attrs), C.byref(opts), int(est.kernel.type),
            C.c_double(est.kernel.scaling_parameter),
            C.c_double(est.kernel.shape_parameter), *tail)
    _lib.check(st, "multi_scale_icp")
    out = RegistrationResult()
    out.transformation = np.array(res.transformation[:]).reshape(4, 4)
    out.inlier_rmse = res.inlier_rmse
    out.fitness = res.fitness
    out.converged = bool(res.converged)
    out.num_iterations = res.num_iterations
    out.correspondence_set = corr[:res.num_correspondences]
    if return_singular_pairs:
        return out, singular_pairs.value
    return out


def icp(source, target, target_normals, max_correspondence_distance,
        init_source_to_target=None, estimation_method=None, criteria=None,
        voxel_size=-1.0, callback_after_iteration=None, allreduce=None,
        source_normals=None, source_colors=None, target_colors=None,
        target_color_gradients=None, device_allreduce=None,
        device_counts=None, level_sharding=False, source_dopplers=None,
        source_directions=None, source_covariances=None,
        target_covariances=None, return_singular_pairs=False):
    """t::pipelines::registration::ICP (Registration.cpp:93-106)."""
    return multi_scale_icp(source, target, target_normals, [voxel_size],
                           [criteria or ICPConvergenceCriteria()],
                           [max_correspondence_distance],
                           init_source_to_target, estimation_method,
                           callback_after_iteration, allreduce, source_normals,
                           source_colors, target_colors,
                           target_color_gradients, device_allreduce,
                           device_counts, level_sharding, source_dopplers,
                           source_directions, source_covariances,
                           target_covariances, return_singular_pairs)


def _check_pair(source, target):
    source = require_cuda(source, "source")
    target = require_cuda(target, "target")
    if source.dtype not in (torch.float32, torch.float64):
        raise ValueError("Only Float32 and Float64 point clouds are supported.")
    if target.dtype != source.dtype:
        raise ValueError("source / target dtype mismatch")
    return source, target


def evaluate_registration(source, target, max_correspondence_distance,
                          transformation=None):
    """t::pipelines::registration::EvaluateRegistration
    (Registration.cpp:64-91)."""
    source, target = _check_pair(source, target)
    T = np.ascontiguousarray(
        np.eye(4) if transformation is None else transformation,
        dtype=np.float64)
    ns = source.shape[0]
    corr = torch.full((ns,), -1, dtype=torch.int64, device="cuda")
    res = _lib.RegistrationResultC()
    _lib.check(_lib.lib().o3dmi_registration_evaluate(
        _lib.ptr(source), ns, _lib.ptr(target), target.shape[0],
        TORCH_TO_O3DMI[source.dtype], C.c_double(max_correspondence_distance),
        _lib.f64p(T), _lib.ptr(corr), C.byref(res), stream()),
        "evaluate_registration")
    out = RegistrationResult()
    out.transformation = np.array(res.transformation[:]).reshape(4, 4)
    out.inlier_rmse = res.inlier_rmse
    out.fitness = res.fitness
    out.correspondence_set = corr
    return out


def get_information_matrix(source, target, max_correspondence_distance,
                           transformation=None):
    """t::pipelines::registration::GetInformationMatrix
    (Registration.cpp:446-486) -> {6,6} float64 (host)."""
    source, target = _check_pair(source, target)
    T = np.ascontiguousarray(
        np.eye(4) if transformation is None else transformation,
        dtype=np.float64)
    G = np.zeros((6, 6), np.float64)
    _lib.check(_lib.lib().o3dmi_registration_information_matrix(
        _lib.ptr(source), source.shape[0], _lib.ptr(target), target.shape[0],
        TORCH_TO_O3DMI[source.dtype], C.c_double(max_correspondence_distance),
        _lib.f64p(T), _lib.f64p(G), stream()), "get_information_matrix")
    return G


def voxel_down_sample(positions, normals, voxel_size):
    """t::geometry::PointCloud::VoxelDownSample (PointCloud.cpp:496-567) for
    positions (+ optional normals): -> (positions {M,3}, normals {M,3}|None),
    voxels in order of first occurrence."""
    positions = require_cuda(positions, "positions")
    n = positions.shape[0]
    out_p = torch.empty_like(positions)
    out_n = None
    if normals is not None:
        normals = require_cuda(normals, "normals")
        out_n = torch.empty_like(normals)
    m = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_voxel_down_sample(
        _lib.ptr(positions), _lib.ptr(normals), n,
        TORCH_TO_O3DMI[positions.dtype], C.c_double(voxel_size),
        _lib.ptr(out_p), _lib.ptr(out_n), C.byref(m), stream()),
        "voxel_down_sample")
    return out_p[:m.value], (None if out_n is None else out_n[:m.value])


def estimate_normals(positions, max_nn=30, radius=None, normals=None):
    """t::geometry::PointCloud::EstimateNormals(max_nn, radius)
    (PointCloud.cpp:856-976): hybrid search when both are given, KNN search
    when radius is None (the reference's default), radius search when max_nn
    is None; returns normals {N,3};
    `normals` (optional) are existing normals whose orientation is kept."""
    positions = require_cuda(positions, "positions")
    if radius is None and max_nn is None:
        raise ValueError("Both max_nn and radius are none.")
    if max_nn is None:
        max_nn = -1      # radius search: every neighbour within radius
    if radius is None:
        radius = -1.0    # KNN search
    if normals is None:
        out = torch.empty_like(positions)
        has = 0
    else:
        out = require_cuda(normals, "normals").clone()
        has = 1
    _lib.check(_lib.lib().o3dmi_pointcloud_estimate_normals(
        _lib.ptr(positions), positions.shape[0],
        TORCH_TO_O3DMI[positions.dtype], int(max_nn), C.c_double(radius),
        _lib.ptr(out), has, stream()), "estimate_normals")
    return out


def knn_search(points, queries, knn):
    """core::nns::NearestNeighborSearch(points).KnnIndex() + KnnSearch(queries,
    knn) -> (indices {Q,k} int32, squared distances {Q,k}), k = min(knn, N)."""
    points = require_cuda(points, "points")
    queries = require_cuda(queries, "queries")
    if queries.dtype != points.dtype:
        raise ValueError("points / queries dtype mismatch")
    n, q = points.shape[0], queries.shape[0]
    k = min(int(knn), n)
    ka = max(k, 1)  # knn <= 0 is rejected by the library, as in the reference
    idx = torch.empty((q, ka), dtype=torch.int32, device="cuda")
    d2 = torch.empty((q, ka), dtype=points.dtype, device="cuda")
    _lib.check(_lib.lib().o3dmi_nns_knn_search(
        _lib.ptr(points), n, _lib.ptr(queries), q,
        TORCH_TO_O3DMI[points.dtype], int(knn), _lib.ptr(idx), _lib.ptr(d2),
        stream()), "knn_search")
    return idx, d2


def estimate_color_gradients(positions, normals, colors, max_nn=30,
                             radius=None):
    """t::geometry::PointCloud::EstimateColorGradients(max_nn, radius)
    (PointCloud.cpp:987-1060) -> gradients {N,3}."""
    positions = require_cuda(positions, "positions")
    normals = require_cuda(normals, "normals")
    colors = require_cuda(colors, "colors")
    if max_nn is None and radius is None:
        raise ValueError("Both max_nn and radius are none.")
    if max_nn is None:
        max_nn = -1      # radius search
    out = torch.empty_like(positions)
    _lib.check(_lib.lib().o3dmi_pointcloud_estimate_color_gradients(
        _lib.ptr(positions), _lib.ptr(normals), _lib.ptr(colors),
        positions.shape[0], TORCH_TO_O3DMI[positions.dtype], int(max_nn),
        C.c_double(-1.0 if radius is None else radius), _lib.ptr(out),
        stream()), "estimate_color_gradients")
    return out


def compute_rmse(estimation_method, source, target, target_normals,
                 correspondences, source_normals=None, source_colors=None,
                 target_colors=None, target_color_gradients=None,
                 source_covariances=None, target_covariances=None):
    """TransformationEstimation*::ComputeRMSE on device tensors (the
    reference's definitions, see o3dmi_registration_compute_rmse; the
    generalized estimator's, on both clouds' covariances {N,3,3}:
    o3dmi_registration_compute_rmse_generalized)."""
    est = estimation_method
    if isinstance(est, TransformationEstimationForGeneralizedICP):
        source, target = _check_pair(source, target)
        corr = require_cuda(correspondences, "correspondences")
        if source_covariances is None or target_covariances is None:
            raise ValueError("GeneralizedICP requires both clouds to have "
                             "covariances.")
        cs = _covariances(source_covariances, "source_covariances", source)
        ct = _covariances(target_covariances, "target_covariances", target)
        out = np.zeros(1, np.float64)
        _lib.check(_lib.lib().o3dmi_registration_compute_rmse_generalized(
            _lib.ptr(source), _lib.ptr(cs), source.shape[0], _lib.ptr(target),
            _lib.ptr(ct), target.shape[0], TORCH_TO_O3DMI[source.dtype],
            _lib.ptr(corr), _lib.f64p(out), stream()), "compute_rmse")
        return float(out[0])
    code = (1 if isinstance(est, TransformationEstimationPointToPoint) else
            2 if isinstance(est, TransformationEstimationSymmetric) else
            3 if isinstance(est, TransformationEstimationForColoredICP) else
            4 if isinstance(est, TransformationEstimationForDopplerICP) else 0)
    source, target = _check_pair(source, target)
    corr = require_cuda(correspondences, "correspondences")
    attrs = _lib.IcpAttributes()
    attrs.lambda_geometric = getattr(est, "lambda_geometric", 0.968)
    keep = [require_cuda(t, "attribute") for t in
            (source_normals, source_colors, target_colors,
             target_color_gradients, target_normals) if t is not None]
    if source_normals is not None:
        attrs.source_normals = source_normals.data_ptr()
    if source_colors is not None:
        attrs.source_colors = source_colors.data_ptr()
    if target_colors is not None:
        attrs.target_colors = target_colors.data_ptr()
    if target_color_gradients is not None:
        attrs.target_color_gradients = target_color_gradients.data_ptr()
    out = C.c_double(0)
    _lib.check(_lib.lib().o3dmi_registration_compute_rmse(
        code, _lib.ptr(source), source.shape[0], _lib.ptr(target),
        _lib.ptr(target_normals), TORCH_TO_O3DMI[source.dtype],
        C.byref(attrs), _lib.ptr(corr), C.byref(out), stream()),
        "compute_rmse")
    del keep
    return out.value


def fixed_radius_search(points, queries, radius):
    """core::nns::NearestNeighborSearch(points).FixedRadiusIndex(radius) +
    FixedRadiusSearch(queries, radius) -> (indices {total} int32, squared
    distances {total}, neighbors_row_splits {Q+1} int64), neighbours of a
    query ascending by (distance, index)."""
    points = require_cuda(points, "points")
    queries = require_cuda(queries, "queries")
    if queries.dtype != points.dtype:
        raise ValueError("points / queries dtype mismatch")
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.o3dmi_nns_create(_lib.ptr(points), points.shape[0],
                                  TORCH_TO_O3DMI[points.dtype],
                                  C.c_double(radius), stream(), C.byref(h)),
               "nns_create")
    try:
        q = queries.shape[0]
        counts = torch.zeros(q, dtype=torch.int32, device="cuda")
        _lib.check(L.o3dmi_nns_radius_count(h, _lib.ptr(queries), q,
                                            _lib.ptr(counts), stream()),
                   "radius_count")
        splits = torch.zeros(q + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(counts, 0, out=splits[1:])
        total = int(splits[-1].item())
        idx = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
        d2 = torch.empty(max(total, 1), dtype=points.dtype, device="cuda")
        _lib.check(L.o3dmi_nns_radius_search(h, _lib.ptr(queries), q,
                                             _lib.ptr(splits), _lib.ptr(idx),
                                             _lib.ptr(d2), stream()),
                   "radius_search")
        torch.cuda.synchronize()
        return idx[:total], d2[:total], splits
    finally:
        L.o3dmi_nns_destroy(h)


def compute_fpfh_feature(positions, normals, max_nn=100, radius=None,
                         indices=None):
    """t::pipelines::registration::ComputeFPFHFeature (Feature.cpp:23-277) ->
    FPFH features {N,33} (with `indices`: one row per distinct index, in
    ascending order). Hybrid search when max_nn and radius are given, KNN
    search when radius is None (the default), radius search when max_nn is
    None. max_nn is limited to 128."""
    positions = require_cuda(positions, "positions")
    if normals is None:
        raise ValueError("The input point cloud has no normal.")
    normals = require_cuda(normals, "normals")
    if normals.dtype != positions.dtype or normals.shape != positions.shape:
        raise ValueError("positions / normals mismatch")
    n = positions.shape[0]
    idx = None
    n_idx = -1
    rows = n
    if indices is not None:
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
        idx = idx.to("cuda").contiguous()
        n_idx = idx.shape[0]
        rows = min(n_idx, n)
    out = torch.zeros((max(rows, 1), 33), dtype=positions.dtype,
                      device="cuda")
    got = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_registration_compute_fpfh_feature(
        _lib.ptr(positions), _lib.ptr(normals), n,
        TORCH_TO_O3DMI[positions.dtype], int(max_nn is not None),
        int(max_nn if max_nn is not None else 0), int(radius is not None),
        C.c_double(radius if radius is not None else 0.0), _lib.ptr(idx),
        n_idx, _lib.ptr(out), C.byref(got), stream()),
        "compute_fpfh_feature")
    return out[:got.value]


def correspondences_from_features(source_features, target_features,
                                  mutual_filter=False,
                                  mutual_consistency_ratio=0.1,
                                  return_fallback=False):
    """t::pipelines::registration::CorrespondencesFromFeatures
    (Feature.cpp:279-333) -> int64 {K,2} pairs (source row, nearest target
    row). Exact float64 distances, ties to the lowest index. With
    return_fallback, also returns whether the mutual filter fell back to all
    pairs (the reference only logs it)."""
    src = require_cuda(source_features, "source_features")
    tgt = require_cuda(target_features, "target_features")
    if src.dtype != tgt.dtype or src.dim() != 2 or tgt.dim() != 2 or \
            src.shape[1] != tgt.shape[1]:
        raise ValueError("feature sets must be {N,D} and {M,D} of one dtype")
    n = src.shape[0]
    out = torch.empty((max(n, 1), 2), dtype=torch.int64, device="cuda")
    k = C.c_int64(0)
    fb = C.c_int(0)
    _lib.check(_lib.lib().o3dmi_registration_correspondences_from_features(
        _lib.ptr(src), n, _lib.ptr(tgt), tgt.shape[0], src.shape[1],
        TORCH_TO_O3DMI[src.dtype], int(bool(mutual_filter)),
        C.c_float(mutual_consistency_ratio), _lib.ptr(out), C.byref(k),
        C.byref(fb), stream()), "correspondences_from_features")
    res = out[:k.value]
    return (res, bool(fb.value)) if return_fallback else res


class RANSACConvergenceCriteria:
    """Registration.h: max_iteration 100000, confidence 0.999."""
    def __init__(self, max_iteration=100000, confidence=0.999):
        self.max_iteration = max_iteration
        self.confidence = confidence


class CorrespondenceCheckerBasedOnEdgeLength:
    """CorrespondenceChecker.cpp:19-40."""
    kind = 0

    def __init__(self, similarity_threshold=0.9):
        self.similarity_threshold = similarity_threshold
        self.threshold = similarity_threshold


class CorrespondenceCheckerBasedOnDistance:
    """CorrespondenceChecker.cpp:42-57."""
    kind = 1

    def __init__(self, distance_threshold):
        self.distance_threshold = distance_threshold
        self.threshold = distance_threshold


class CorrespondenceCheckerBasedOnNormal:
    """CorrespondenceChecker.cpp:59-83; passes when either cloud has no
    normals."""
    kind = 2

    def __init__(self, normal_angle_threshold):
        self.normal_angle_threshold = normal_angle_threshold
        self.threshold = normal_angle_threshold


def _ransac_options(checkers, criteria, seed, batch_size):
    checkers = list(checkers or [])
    if len(checkers) > 3:
        raise ValueError("at most one checker of each kind")
    criteria = criteria or RANSACConvergenceCriteria()
    opt = _lib.RansacOptionsC()
    opt.num_checkers = len(checkers)
    for k, c in enumerate(checkers):
        if not hasattr(c, "kind"):
            raise ValueError("unsupported correspondence checker %r" % (c,))
        opt.checker_types[k] = c.kind
        opt.checker_thresholds[k] = float(c.threshold)
    opt.max_iteration = int(criteria.max_iteration)
    opt.confidence = float(criteria.confidence)
    opt.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    opt.batch_size = int(batch_size)
    return opt


def _ransac_estimation(estimation_method):
    est = estimation_method or TransformationEstimationPointToPoint()
    code = (1 if isinstance(est, TransformationEstimationPointToPoint) else
            2 if isinstance(est, TransformationEstimationSymmetric) else
            3 if isinstance(est, TransformationEstimationForColoredICP) else 0)
    return code, int(bool(getattr(est, "with_scaling", False)))


def _ransac_normals(source, target, source_normals, target_normals):
    sn = tn = None
    if source_normals is not None:
        sn = require_cuda(source_normals, "source_normals")
        if sn.dtype != source.dtype or sn.shape != source.shape:
            raise ValueError("source / source_normals mismatch")
    if target_normals is not None:
        tn = require_cuda(target_normals, "target_normals")
        if tn.dtype != target.dtype or tn.shape != target.shape:
            raise ValueError("target / target_normals mismatch")
    return sn, tn


def _ransac_result(res, info, corr):
    out = RegistrationResult()
    out.transformation = np.array(res.transformation[:]).reshape(4, 4)
    out.inlier_rmse = res.inlier_rmse
    out.fitness = res.fitness
    out.correspondence_set = corr
    out.best_iteration = info.best_iteration
    out.num_validations = info.num_validations
    out.final_iteration_bound = info.final_iteration_bound
    out.iterations_run = info.iterations_run
    out.num_batches = info.num_batches
    return out


def registration_ransac_based_on_correspondence(
        source, target, corres, max_correspondence_distance,
        estimation_method=None, ransac_n=3, checkers=(), criteria=None,
        seed=0, source_normals=None, target_normals=None, batch_size=0):
    """Legacy pipelines::registration::RegistrationRANSACBasedOnCorrespondence
    (Registration.cpp:344-380) on device tensors: `corres` int64 {K,2} (source
    row, target row). The reference loop as one thread runs it over a
    stateless sample stream keyed by `seed` (rules 1-7 in o3d_mi355x.h); the
    result does not depend on `batch_size` (0 = the library's choice). The
    normals are read by CorrespondenceCheckerBasedOnNormal only. Returns a
    RegistrationResult with best_iteration (-1: none), num_validations and
    final_iteration_bound as extra attributes."""
    source, target = _check_pair(source, target)
    corres = require_cuda(corres, "corres")
    if corres.dtype != torch.int64 or corres.dim() != 2 or \
            corres.shape[1] != 2:
        raise ValueError("corres must be int64 {K,2}")
    sn, tn = _ransac_normals(source, target, source_normals, target_normals)
    code, scaling = _ransac_estimation(estimation_method)
    opt = _ransac_options(checkers, criteria, seed, batch_size)
    ns = source.shape[0]
    corr = torch.full((max(ns, 1),), -1, dtype=torch.int64, device="cuda")
    res = _lib.RegistrationResultC()
    info = _lib.RansacInfoC()
    _lib.check(_lib.lib().o3dmi_registration_ransac_correspondence(
        _lib.ptr(source), ns, _lib.ptr(target), target.shape[0],
        _lib.ptr(sn), _lib.ptr(tn), TORCH_TO_O3DMI[source.dtype],
        _lib.ptr(corres), corres.shape[0],
        C.c_double(max_correspondence_distance), code, scaling, int(ransac_n),
        C.byref(opt), _lib.ptr(corr), C.byref(res), C.byref(info), stream()),
        "registration_ransac_based_on_correspondence")
    return _ransac_result(res, info, corr[:ns])


def registration_ransac_based_on_feature_matching(
        source, target, source_features, target_features, mutual_filter,
        max_correspondence_distance, estimation_method=None, ransac_n=3,
        checkers=(), criteria=None, seed=0, source_normals=None,
        target_normals=None, batch_size=0):
    """Legacy RegistrationRANSACBasedOnFeatureMatching (Registration.cpp:
    382-406): correspondences_from_features(source_features, target_features,
    mutual_filter) followed by the function above. Features {N,D}, row r of
    point r."""
    source, target = _check_pair(source, target)
    fs = require_cuda(source_features, "source_features")
    ft = require_cuda(target_features, "target_features")
    if fs.dtype != ft.dtype or fs.dim() != 2 or ft.dim() != 2 or \
            fs.shape[1] != ft.shape[1] or fs.shape[0] != source.shape[0] or \
            ft.shape[0] != target.shape[0]:
        raise ValueError("features must be {N,D} / {M,D} of one dtype, one "
                         "row per point")
    sn, tn = _ransac_normals(source, target, source_normals, target_normals)
    code, scaling = _ransac_estimation(estimation_method)
    opt = _ransac_options(checkers, criteria, seed, batch_size)
    ns = source.shape[0]
    corr = torch.full((max(ns, 1),), -1, dtype=torch.int64, device="cuda")
    res = _lib.RegistrationResultC()
    info = _lib.RansacInfoC()
    _lib.check(_lib.lib().o3dmi_registration_ransac_feature_matching(
        _lib.ptr(source), ns, _lib.ptr(target), target.shape[0],
        _lib.ptr(sn), _lib.ptr(tn), TORCH_TO_O3DMI[source.dtype],
        _lib.ptr(fs), _lib.ptr(ft), fs.shape[1], TORCH_TO_O3DMI[fs.dtype],
        int(bool(mutual_filter)), C.c_double(max_correspondence_distance),
        code, scaling, int(ransac_n), C.byref(opt), _lib.ptr(corr),
        C.byref(res), C.byref(info), stream()),
        "registration_ransac_based_on_feature_matching")
    return _ransac_result(res, info, corr[:ns])


class FastGlobalRegistrationOption:
    """FastGlobalRegistration.h: upstream's fields and defaults, plus `seed`
    (the tuple test draws from a stateless stream keyed by it, where upstream
    uses its global Mersenne engine)."""
    def __init__(self, division_factor=1.4, use_absolute_scale=False,
                 decrease_mu=True, maximum_correspondence_distance=0.025,
                 iteration_number=64, tuple_scale=0.95,
                 maximum_tuple_count=1000, tuple_test=True, seed=0):
        self.division_factor = division_factor
        self.use_absolute_scale = use_absolute_scale
        self.decrease_mu = decrease_mu
        self.maximum_correspondence_distance = maximum_correspondence_distance
        self.iteration_number = iteration_number
        self.tuple_scale = tuple_scale
        self.maximum_tuple_count = maximum_tuple_count
        self.tuple_test = tuple_test
        self.seed = seed


def _fgr_options(option):
    option = option or FastGlobalRegistrationOption()
    opt = _lib.FgrOptionsC()
    opt.division_factor = float(option.division_factor)
    opt.use_absolute_scale = int(bool(option.use_absolute_scale))
    opt.decrease_mu = int(bool(option.decrease_mu))
    opt.maximum_correspondence_distance = float(
        option.maximum_correspondence_distance)
    opt.iteration_number = int(option.iteration_number)
    opt.tuple_scale = float(option.tuple_scale)
    opt.maximum_tuple_count = int(option.maximum_tuple_count)
    opt.tuple_test = int(bool(option.tuple_test))
    opt.seed = int(option.seed) & 0xFFFFFFFFFFFFFFFF
    return opt


def _fgr_result(res, info, corr):
    out = RegistrationResult()
    out.transformation = np.array(res.transformation[:]).reshape(4, 4)
    out.inlier_rmse = res.inlier_rmse
    out.fitness = res.fitness
    out.correspondence_set = corr
    names = [f for f, _ in _lib.FgrInfoC._fields_]
    return out, {k: getattr(info, k) for k in names}


def registration_fgr_based_on_correspondence(source, target, corres,
                                             option=None):
    """Legacy pipelines::registration::
    FastGlobalRegistrationBasedOnCorrespondence on device tensors: `corres`
    int64 {K,2} (source row, target row). Rules 1-6 of "Fast Global
    Registration" in o3d_mi355x.h / o3d_mi355x_host.h. Returns
    (RegistrationResult, info): info is a dict of o3dmi_fgr_info_t (n_initial,
    n_trials, n_tuples, n_used, scale_global, final_par, swapped,
    failed_solves, form)."""
    source, target = _check_pair(source, target)
    corres = require_cuda(corres, "corres")
    if corres.dtype != torch.int64 or corres.dim() != 2 or \
            corres.shape[1] != 2:
        raise ValueError("corres must be int64 {K,2}")
    opt = _fgr_options(option)
    ns = source.shape[0]
    corr = torch.full((max(ns, 1),), -1, dtype=torch.int64, device="cuda")
    res = _lib.RegistrationResultC()
    info = _lib.FgrInfoC()
    _lib.check(_lib.lib().o3dmi_registration_fgr_correspondence(
        _lib.ptr(source), ns, _lib.ptr(target), target.shape[0],
        TORCH_TO_O3DMI[source.dtype], _lib.ptr(corres), corres.shape[0],
        C.byref(opt), _lib.ptr(corr), C.byref(res), C.byref(info), stream()),
        "registration_fgr_based_on_correspondence")
    return _fgr_result(res, info, corr[:ns])


def registration_fgr_based_on_feature_matching(source, target,
                                               source_features,
                                               target_features, option=None):
    """Legacy FastGlobalRegistrationBasedOnFeatureMatching: the cross-checked
    nearest feature rows (no fall-back to all pairs), the tuple test, then as
    above. Features {N,D} / {M,D} of one dtype, row r of point r. Returns
    (RegistrationResult, info)."""
    source, target = _check_pair(source, target)
    fs = require_cuda(source_features, "source_features")
    ft = require_cuda(target_features, "target_features")
    if fs.dtype != ft.dtype or fs.dim() != 2 or ft.dim() != 2 or \
            fs.shape[1] != ft.shape[1] or fs.shape[0] != source.shape[0] or \
            ft.shape[0] != target.shape[0]:
        raise ValueError("features must be {N,D} / {M,D} of one dtype, one "
                         "row per point")
    opt = _fgr_options(option)
    ns = source.shape[0]
    corr = torch.full((max(ns, 1),), -1, dtype=torch.int64, device="cuda")
    res = _lib.RegistrationResultC()
    info = _lib.FgrInfoC()
    _lib.check(_lib.lib().o3dmi_registration_fgr_feature_matching(
        _lib.ptr(source), ns, _lib.ptr(target), target.shape[0],
        TORCH_TO_O3DMI[source.dtype], _lib.ptr(fs), _lib.ptr(ft),
        fs.shape[1], TORCH_TO_O3DMI[fs.dtype], C.byref(opt), _lib.ptr(corr),
        C.byref(res), C.byref(info), stream()),
        "registration_fgr_based_on_feature_matching")
    return _fgr_result(res, info, corr[:ns])
