"""ctypes binding of the C ABI in include/o3d_mi355x.h.

The HIP library is mandatory: there is no CPU or PyTorch fallback. If
libo3d_mi355x.so is missing or fails to load, importing a compute entry point
raises immediately.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# O3DMI_LIB: another build of the same library (A/B measurements of two
# builds on one box); the default is the in-tree build.
SO_PATH = os.environ.get("O3DMI_LIB") or os.path.join(
    _HERE, "lib", "libo3d_mi355x.so")

OK = 0
F32, F64, U16, U8, I32, I64 = 0, 1, 2, 3, 4, 5
I8, I16, U32, U64, BOOL = 6, 7, 8, 9, 10

_vp = C.c_void_p
_i64 = C.c_int64
_i32 = C.c_int
_f = C.c_float
_d = C.c_double
_dp = C.POINTER(C.c_double)

# name -> (restype, argtypes). Kept in one table so that tests can check that
# every symbol the header declares is exported.
PROTOTYPES = {
    "o3dmi_abi_version": (_i32, []),
    "o3dmi_status_string": (C.c_char_p, [_i32]),
    "o3dmi_last_error": (C.c_char_p, []),
    "o3dmi_device_info": (_i32, [C.c_char_p, C.c_size_t, C.POINTER(_i32),
                                 C.POINTER(_i64)]),
    "o3dmi_release_cached_memory": (_i32, []),
    "o3dmi_hash_create": (_i32, [_i64, _i32, C.POINTER(_i64), _vp,
                                 C.POINTER(_vp)]),
    "o3dmi_hash_destroy": (_i32, [_vp]),
    "o3dmi_hash_clear": (_i32, [_vp, _vp]),
    "o3dmi_hash_activate": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "o3dmi_hash_insert": (_i32, [_vp, _vp, C.POINTER(_vp), _i64, _vp, _vp,
                                 _vp]),
    "o3dmi_hash_find": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "o3dmi_hash_erase": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "o3dmi_hash_size": (_i32, [_vp, _vp, C.POINTER(_i64)]),
    "o3dmi_hash_capacity": (_i64, [_vp]),
    "o3dmi_hash_bucket_count": (_i64, [_vp]),
    "o3dmi_hash_active_indices": (_i32, [_vp, _vp, _vp, C.POINTER(_i64)]),
    "o3dmi_hash_reserve": (_i32, [_vp, _i64, _vp]),
    "o3dmi_hash_set_ownership": (_i32, [_vp, _i32, _i32]),
    "o3dmi_block_owner": (_i32, [C.POINTER(_i32), _i32]),
    "o3dmi_hash_key_buffer": (_vp, [_vp]),
    "o3dmi_hash_value_buffer": (_vp, [_vp, _i32]),
    "o3dmi_vbg_depth_touch": (_i32, [_vp, _vp, _i32, _i32, _i32, _dp, _dp,
                                     _vp, _i64, _vp, _i32, _f, _f, _f, _f,
                                     _i32, _vp]),
    "o3dmi_vbg_pointcloud_touch": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp,
                                          _i32, _f, _f, _vp]),
    "o3dmi_vbg_voxel_coordinates_and_flattened_indices": (
        _i32, [_vp, _i64, _vp, _i32, _f, _vp, _vp, _vp]),
    "o3dmi_vbg_voxel_indices": (_i32, [_vp, _i64, _i32, _vp, _vp]),
    "o3dmi_vbg_voxel_coordinates": (_i32, [_vp, _i64, _vp, _i64, _i32, _vp,
                                           _vp, _vp]),
    "o3dmi_vbg_integrate": (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _i32,
                                   _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32,
                                   _dp, _dp, _dp, _i32, _f, _f, _f, _f, _vp]),
    "o3dmi_vbg_touch_activate": (_i32, [_vp, _vp, _i32, _i32, _i32, _dp, _dp,
                                        _vp, _i64, _vp, _i32, _f, _f, _f, _f,
                                        _i32, _i32, _vp]),
    "o3dmi_vbg_estimate_range": (_i32, [_vp, _i64, _vp, _dp, _dp, _i32, _i32,
                                        _i32, _i64, _f, _f, _f, _vp]),
    "o3dmi_vbg_estimate_range_dev": (_i32, [_vp, _i64, _vp, _vp, _dp, _dp,
                                            _i32, _i32, _i32, _i64, _f, _f,
                                            _f, _vp]),
    "o3dmi_vbg_raycast": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp] + [_vp] * 10 +
                          [_dp, _dp, _i32, _i32, _i32, _f, _f, _f, _f, _f, _f,
                           _i32, _vp]),
    "o3dmi_vbg_raycast_rows": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp] +
                               [_vp] * 10 +
                               [_dp, _dp, _i32, _i32, _i32, _i32, _i32, _f, _f,
                                _f, _f, _f, _f, _i32, _vp]),
    "o3dmi_unproject": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _dp,
                               _dp, _f, _f, _i64, _vp]),
    "o3dmi_unproject_pair": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _dp,
                                    _vp, _i32, _vp, _vp, _vp, _vp, _dp,
                                    _i32, _i32, _dp, _f, _f, _i64, _vp]),
    "o3dmi_nns_create": (_i32, [_vp, _i64, _i32, _d, _vp, C.POINTER(_vp)]),
    "o3dmi_nns_destroy": (_i32, [_vp]),
    "o3dmi_nns_hybrid_search_k1": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp,
                                          _vp]),
    "o3dmi_nns_hybrid_search": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp,
                                       _vp]),
    "o3dmi_pointcloud_estimate_covariances": (_i32, [_vp, _vp, _vp, _i64, _i32,
                                                     _i32, _vp, _vp]),
    "o3dmi_pointcloud_normals_from_covariances": (_i32, [_vp, _i64, _i32, _vp,
                                                         _i32, _vp]),
    "o3dmi_icp_p2plane_accumulate": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32,
                                            _i32, _d, _d, _vp, _vp]),
    "o3dmi_icp_search_accumulate": (_i32, [_vp, _vp, _vp, _i64, _i32, _d, _d,
                                           _vp, _vp, _vp]),
    "o3dmi_transform_points": (_i32, [_dp, _vp, _i64, _i32, _vp]),
    "o3dmi_transform_normals": (_i32, [_dp, _vp, _i64, _i32, _vp]),
    "o3dmi_decode_and_solve6x6": (_i32, [_dp, _dp, C.POINTER(_f),
                                         C.POINTER(_i32)]),
    "o3dmi_pose_to_transformation": (None, [_dp, _dp]),
    "o3dmi_transformation_to_pose": (None, [_dp, _dp]),
    "o3dmi_vbg_extract_points": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _i32,
                                        _i32, _f, _f, _vp, _vp, _vp, _i64,
                                        C.POINTER(_i64), _vp]),
    "o3dmi_vbg_extract_mesh": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _i32,
                                      _i32, _f, _f, _vp, _vp, _vp, _vp, _i64,
                                      C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "o3dmi_sort_indices": (_i32, [_vp, _i64, _vp]),
    "o3dmi_image_clip_transform": (_i32, [_vp, _i32, _i32, _i32, _f, _f, _f,
                                          _f, _vp, _vp]),
    "o3dmi_image_pyrdown_depth": (_i32, [_vp, _i32, _i32, _f, _f, _vp, _vp]),
    "o3dmi_image_create_vertex_map": (_i32, [_vp, _i32, _i32, _dp, _f, _vp,
                                             _vp]),
    "o3dmi_image_create_normal_map": (_i32, [_vp, _i32, _i32, _f, _vp, _vp]),
    "o3dmi_image_to_float": (_i32, [_vp, _i32, _i64, _d, _d, _vp, _vp]),
    "o3dmi_image_rgb_to_gray": (_i32, [_vp, _i32, _i64, _vp, _vp]),
    "o3dmi_image_rgb_to_intensity": (_i32, [_vp, _i32, _i64, _vp, _vp]),
    "o3dmi_image_filter_bilateral": (_i32, [_vp, _i32, _i32, _i32, _f, _f,
                                            _vp, _vp]),
    "o3dmi_image_filter_gaussian": (_i32, [_vp, _i32, _i32, _i32, _f, _vp,
                                           _vp]),
    "o3dmi_image_filter_sobel": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp]),
    "o3dmi_image_resize_half_nearest": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "o3dmi_image_pyrdown": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "o3dmi_odometry_p2plane_level": (_i32, [_vp, _vp, _i32, _i32, _dp, _vp,
                                            _vp, _vp, _vp, _vp, _f, _vp]),
    "o3dmi_image_clip_transform_pair": (_i32, [_vp, _i32, _vp, _i32, _i32,
                                               _i32, _f, _f, _f, _f, _vp, _vp,
                                               _vp]),
    "o3dmi_odometry_sums_scratch_doubles": (_i32, []),
    "o3dmi_odometry_sums": (_i32, [_i32, _i32, _i32] + [_vp] * 11 +
                            [_dp, _dp, _f, _f, _f, _vp, _vp, _vp]),
    "o3dmi_odometry_information": (_i32, [_i32, _i32, _vp, _vp, _dp, _dp, _f,
                                          _dp, _vp]),
}

# include/o3d_mi355x_host.h
class IcpCriteria(C.Structure):
    _fields_ = [("relative_fitness", _d), ("relative_rmse", _d),
                ("max_iteration", _i32)]


class RegistrationResultC(C.Structure):
    _fields_ = [("transformation", _d * 16), ("inlier_rmse", _d),
                ("fitness", _d), ("converged", _i32),
                ("num_iterations", _i32), ("num_correspondences", _i64)]


class OdometryCriteriaC(C.Structure):
    _fields_ = [("max_iteration", _i32), ("relative_rmse", _d),
                ("relative_fitness", _d)]


class OdometryResultC(C.Structure):
    _fields_ = [("transformation", _d * 16), ("inlier_rmse", _d),
                ("fitness", _d), ("num_iterations", _i32)]


class RansacOptionsC(C.Structure):
    _fields_ = [("num_checkers", _i32), ("checker_types", _i32 * 3),
                ("checker_thresholds", _d * 3), ("max_iteration", _i32),
                ("confidence", _d), ("seed", C.c_uint64),
                ("batch_size", _i32)]


class RansacInfoC(C.Structure):
    _fields_ = [("best_iteration", _i64), ("num_validations", _i64),
                ("final_iteration_bound", _i64), ("iterations_run", _i64),
                ("num_batches", _i64)]


class FgrOptionsC(C.Structure):
    _fields_ = [("division_factor", _d), ("use_absolute_scale", _i32),
                ("decrease_mu", _i32),
                ("maximum_correspondence_distance", _d),
                ("iteration_number", _i32), ("tuple_scale", _d),
                ("maximum_tuple_count", _i32), ("tuple_test", _i32),
                ("seed", C.c_uint64)]


class FgrInfoC(C.Structure):
    _fields_ = [("n_initial", _i64), ("n_trials", _i64), ("n_tuples", _i64),
                ("n_used", _i64), ("scale_global", _d), ("final_par", _d),
                ("swapped", _i32), ("failed_solves", _i32), ("form", _i32)]


class SegmentPlaneInfoC(C.Structure):
    _fields_ = [("best_iteration", _i64), ("iterations_counted", _i64),
                ("final_break_iteration", _i64), ("fitness", _d),
                ("inlier_rmse", _d)]


class MetricsRawC(C.Structure):
    _fields_ = [("sum", _d * 2), ("max", _d * 2),
                ("counts", C.POINTER(_i64)),
                ("second_pass_queries", _i64 * 2)]


class IcpAttributes(C.Structure):
    _fields_ = [("source_normals", _vp), ("source_colors", _vp),
                ("target_colors", _vp), ("target_color_gradients", _vp),
                ("lambda_geometric", _d)]


ICP_CALLBACK = C.CFUNCTYPE(None, _i64, _i64, _i64, _d, _d, _dp, _vp)
ALLREDUCE_SUM = C.CFUNCTYPE(_i32, _dp, _i32, _vp)
ALLREDUCE_DEVICE = C.CFUNCTYPE(_i32, _vp, _i32, _vp, _vp)


class IcpOptions(C.Structure):
    _fields_ = [("ns_dev", _vp), ("nt_dev", _vp),
                ("device_allreduce", ALLREDUCE_DEVICE),
                ("device_allreduce_user", _vp), ("level_sharding", _i32)]


class IcpDoppler(C.Structure):
    _fields_ = [("source_dopplers", _vp), ("source_directions", _vp),
                ("transform_vehicle_to_sensor", _d * 16), ("period", _d),
                ("lambda_doppler", _d), ("reject_dynamic_outliers", _i32),
                ("doppler_outlier_threshold", _d),
                ("outlier_rejection_min_iteration", _i32),
                ("geometric_robust_loss_min_iteration", _i32),
                ("doppler_robust_loss_min_iteration", _i32),
                ("geometric_kernel", _i32),
                ("geometric_scaling_parameter", _d),
                ("geometric_shape_parameter", _d), ("doppler_kernel", _i32),
                ("doppler_scaling_parameter", _d),
                ("doppler_shape_parameter", _d)]


class IcpGeneralized(C.Structure):
    _fields_ = [("source_covariances", _vp), ("target_covariances", _vp),
                ("source_normals", _vp), ("epsilon", _d),
                ("robust_kernel", _i32), ("scaling_parameter", _d),
                ("shape_parameter", _d),
                ("singular_pairs_out", C.POINTER(_i64))]


PROTOTYPES.update({
    "o3dmi_registration_multiscale_icp_generalized": (
        _i32, [_vp, _i64, _vp, _vp, _i64, _i32, _i32, _dp,
               C.POINTER(IcpCriteria), _dp, _dp, C.POINTER(IcpGeneralized),
               C.POINTER(IcpOptions), ICP_CALLBACK, _vp, ALLREDUCE_SUM, _vp,
               _vp, C.POINTER(RegistrationResultC), _vp]),
    "o3dmi_icp_generalized_accumulate": (
        _i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _dp, _i32, _d, _d,
               _vp, _vp]),
    "o3dmi_registration_compute_rmse_generalized": (
        _i32, [_vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _dp, _vp]),
    "o3dmi_pointcloud_covariances_from_normals": (
        _i32, [_vp, _i64, _i32, _d, _vp, _vp]),
    "o3dmi_registration_multiscale_icp_doppler": (
        _i32, [_vp, _i64, _vp, _vp, _i64, _i32, _i32, _dp,
               C.POINTER(IcpCriteria), _dp, _dp, C.POINTER(IcpDoppler),
               C.POINTER(IcpOptions), ICP_CALLBACK, _vp, ALLREDUCE_SUM, _vp,
               _vp, C.POINTER(RegistrationResultC), _vp]),
    "o3dmi_icp_doppler_accumulate": (
        _i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _dp, _dp, _dp,
               _dp, _d, _i32, _d, _i32, _d, _d, _i32, _d, _d, _d, _vp, _vp]),
    "o3dmi_registration_multiscale_icp": (
        _i32, [_vp, _i64, _vp, _vp, _i64, _i32, _i32, _dp,
               C.POINTER(IcpCriteria), _dp, _dp, _i32, _d, _d, ICP_CALLBACK,
               _vp, ALLREDUCE_SUM, _vp, _vp, C.POINTER(RegistrationResultC),
               _vp]),
    "o3dmi_registration_multiscale_icp_ex": (
        _i32, [_vp, _i64, _vp, _vp, _i64, _i32, _i32, _dp,
               C.POINTER(IcpCriteria), _dp, _dp, _i32,
               C.POINTER(IcpAttributes), C.POINTER(IcpOptions), _i32, _d, _d,
               ICP_CALLBACK, _vp, ALLREDUCE_SUM, _vp, _vp,
               C.POINTER(RegistrationResultC), _vp]),
    "o3dmi_icp_colored_accumulate": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _i64, _i32, _d, _i32, _d, _d, _vp,
                                            _vp]),
    "o3dmi_pointcloud_color_gradients_from_neighbors": (
        _i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "o3dmi_pointcloud_estimate_color_gradients": (
        _i32, [_vp, _vp, _vp, _i64, _i32, _i32, _d, _vp, _vp]),
    "o3dmi_nns_radius_count": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "o3dmi_nns_radius_search": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "o3dmi_nns_radius_covariances": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "o3dmi_nns_knn_search": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _vp,
                                    _vp, _vp]),
    "o3dmi_registration_compute_rmse": (
        _i32, [_i32, _vp, _i64, _vp, _vp, _i32, C.POINTER(IcpAttributes), _vp,
               C.POINTER(_d), _vp]),
    "o3dmi_registration_evaluate": (
        _i32, [_vp, _i64, _vp, _i64, _i32, _d, _dp, _vp,
               C.POINTER(RegistrationResultC), _vp]),
    "o3dmi_registration_information_matrix": (
        _i32, [_vp, _i64, _vp, _i64, _i32, _d, _dp, _dp, _vp]),
    "o3dmi_icp_information_accumulate": (_i32, [_vp, _vp, _i64, _i32, _vp,
                                                _vp]),
    "o3dmi_icp_symmetric_accumulate": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64,
                                              _i32, _dp, _dp, _i32, _d, _d,
                                              _vp, _vp]),
    "o3dmi_symmetric_pose_to_transformation": (None, [_dp, _dp, _dp, _dp]),
    "o3dmi_icp_p2point_accumulate": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp,
                                            _vp]),
    "o3dmi_icp_search_accumulate_p2point": (_i32, [_vp, _vp, _i64, _vp, _vp,
                                                   _vp]),
    "o3dmi_compute_rt_p2point": (_i32, [_dp, _dp, _dp]),
    "o3dmi_fpfh_from_neighbors": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp,
                                         _vp, _i32, _i64, _vp, _vp, _vp,
                                         C.POINTER(_i64), _vp]),
    "o3dmi_registration_compute_fpfh_feature": (
        _i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _d, _vp, _i64, _vp,
               C.POINTER(_i64), _vp]),
    "o3dmi_registration_correspondences_from_features": (
        _i32, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _f, _vp,
               C.POINTER(_i64), C.POINTER(_i32), _vp]),
    "o3dmi_ransac_hypotheses": (
        _i32, [C.c_uint64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i32,
               _vp, _i64, _i32, _i32, C.POINTER(_i32), _dp, _vp, _vp, _vp,
               _vp]),
    "o3dmi_ransac_score_scratch_bytes": (C.c_size_t, [_i64, _i64]),
    "o3dmi_ransac_score": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp,
                                  _i64, _vp, _vp, _vp, _vp, _vp]),
    "o3dmi_registration_ransac_correspondence": (
        _i32, [_vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _i64, _d, _i32,
               _i32, _i32, C.POINTER(RansacOptionsC), _vp,
               C.POINTER(RegistrationResultC), C.POINTER(RansacInfoC), _vp]),
    "o3dmi_registration_ransac_feature_matching": (
        _i32, [_vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _i32, _i32,
               _i32, _d, _i32, _i32, _i32, C.POINTER(RansacOptionsC), _vp,
               C.POINTER(RegistrationResultC), C.POINTER(RansacInfoC), _vp]),
    "o3dmi_fgr_tuple_test": (
        _i32, [C.c_uint64, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _d, _i64,
               _vp, C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "o3dmi_fgr_optimize_scratch_bytes": (C.c_size_t, [_i64]),
    "o3dmi_fgr_optimize": (
        _i32, [_vp, _i64, _vp, _i64, _vp, _i64, _d, _d, _i32, _d, _i32, _vp,
               _vp, _vp]),
    "o3dmi_registration_fgr_correspondence": (
        _i32, [_vp, _i64, _vp, _i64, _i32, _vp, _i64,
               C.POINTER(FgrOptionsC), _vp, C.POINTER(RegistrationResultC),
               C.POINTER(FgrInfoC), _vp]),
    "o3dmi_registration_fgr_feature_matching": (
        _i32, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i32,
               C.POINTER(FgrOptionsC), _vp, C.POINTER(RegistrationResultC),
               C.POINTER(FgrInfoC), _vp]),
    "o3dmi_fill_in_rigid_alignment_term": (
        _i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _f,
               _vp]),
    "o3dmi_slac_rigid_terms": (
        _i32, [C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i64), _i32,
               C.POINTER(_i32), C.POINTER(_vp), C.POINTER(_i64), _i32, _dp,
               _f, _vp, _vp]),
    "o3dmi_slac_correspondence_set": (
        _i32, [_vp, _i64, _vp, _i64, _i32, _i32, _dp, _dp, _dp, _f, _f, _vp,
               C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_f),
               C.POINTER(_i32), _vp]),
    "o3dmi_slac_rigid_optimize": (
        _i32, [C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i64), _i32, _dp,
               C.POINTER(_i32), _dp, _i32, _i32, _f, _f, _dp,
               C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "o3dmi_control_grid_create": (_i32, [_f, _i64, _vp, C.POINTER(_vp)]),
    "o3dmi_control_grid_create_from": (_i32, [_f, _vp, _vp, _i64, _vp,
                                              C.POINTER(_vp)]),
    "o3dmi_control_grid_destroy": (_i32, [_vp]),
    "o3dmi_control_grid_touch": (_i32, [_vp, _vp, _i64, _vp]),
    "o3dmi_control_grid_compactify": (_i32, [_vp, _vp]),
    "o3dmi_control_grid_size": (_i32, [_vp, _vp, C.POINTER(_i64)]),
    "o3dmi_control_grid_anchor_idx": (_i32, [_vp]),
    "o3dmi_control_grid_grid_size": (_f, [_vp]),
    "o3dmi_control_grid_hashmap": (_vp, [_vp]),
    "o3dmi_control_grid_init_positions": (_i32, [_vp, _vp, _vp]),
    "o3dmi_control_grid_curr_positions": (_vp, [_vp]),
    "o3dmi_control_grid_neighbor_grid_map": (_i32, [_vp, _vp, _vp, _vp,
                                                    C.POINTER(_i64), _vp]),
    "o3dmi_control_grid_parameterize": (
        _i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
               C.POINTER(_i64), _vp]),
    "o3dmi_control_grid_deform": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp,
                                         _vp]),
    "o3dmi_project_to_depth_image": (_i32, [_vp, _i64, _i32, _i32, _dp, _dp,
                                            _f, _f, _vp, _vp]),
    "o3dmi_project_to_rgbd_image": (_i32, [_vp, _vp, _i64, _i32, _i32, _dp,
                                           _dp, _f, _f, _vp, _vp, _vp]),
    "o3dmi_control_grid_deform_depth_image": (
        _i32, [_vp, _vp, _i32, _i32, _i32, _dp, _dp, _f, _f, _vp, _vp]),
    "o3dmi_control_grid_deform_rgbd_image": (
        _i32, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _dp, _dp, _f, _f, _vp,
               _vp, _vp]),
    "o3dmi_fill_in_slac_alignment_term": (
        _i32, [_vp, _vp, _vp, _i64] + [_vp] * 9 + [_i64, _i32, _i32, _i32, _f,
                                                   _vp]),
    "o3dmi_fill_in_slac_regularizer_term": (
        _i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _f,
               _i32, _i32, _vp]),
    "o3dmi_slac_solve_spd": (_i32, [_vp, _vp, _i64, _vp]),
    "o3dmi_slac_optimize": (
        _i32, [C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i64), _i32, _dp,
               C.POINTER(_i32), _dp, _i32, _vp, _i32, _f, _f, _f, _dp, _dp,
               C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64),
               C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_estimate_normals": (_i32, [_vp, _i64, _i32, _i32, _d,
                                                 _vp, _i32, _vp]),
    "o3dmi_voxel_down_sample": (_i32, [_vp, _vp, _i64, _i32, _d, _vp, _vp,
                                       C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_select_by_mask": (
        _i32, [_i64, _vp, _i32, _i32, C.POINTER(_vp), C.POINTER(_i64),
               C.POINTER(_vp), C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_select_by_index": (
        _i32, [_i64, _vp, _i64, _i32, _i32, _i32, C.POINTER(_vp),
               C.POINTER(_i64), C.POINTER(_vp), C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_remove_non_finite_points": (
        _i32, [_vp, _i64, _i32, _i32, _i32, _vp, C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_remove_duplicated_points": (
        _i32, [_vp, _i64, _i32, _vp, C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_remove_radius_outliers": (
        _i32, [_vp, _i64, _i32, _i64, _d, _vp, C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_remove_statistical_outliers": (
        _i32, [_vp, _i64, _i32, _i64, _d, _vp, _vp, _dp, C.POINTER(_i64),
               _vp]),
    "o3dmi_pointcloud_cluster_dbscan": (
        _i32, [_vp, _i64, _i32, _d, _i64, _vp, C.POINTER(_i64),
               C.POINTER(_i64), _vp]),
    "o3dmi_plane_sample": (None, [C.c_uint64, _i64, _i32, _i64,
                                  C.POINTER(_i64)]),
    "o3dmi_plane_score": (_i32, [_vp, _i64, _i32, _vp, _i64, _d, _vp, _vp,
                                 _vp]),
    "o3dmi_pointcloud_segment_plane": (
        _i32, [_vp, _i64, _i32, _d, _i32, _i64, _d, C.c_uint64, _dp, _vp,
               C.POINTER(_i64), C.POINTER(SegmentPlaneInfoC), _vp]),
    "o3dmi_pointcloud_farthest_point_order": (
        _i32, [_vp, _i64, _i32, _i64, _i64, _i32, _vp, _vp]),
    "o3dmi_pointcloud_farthest_point_capacity": (_i64, [_i32]),
    "o3dmi_pointcloud_farthest_point_down_sample": (
        _i32, [_vp, _i64, _i32, _i64, _i64, _vp, _vp, C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_uniform_down_sample": (
        _i32, [_i64, _i64, _i32, C.POINTER(_vp), C.POINTER(_i64),
               C.POINTER(_vp), C.POINTER(_i64), _vp]),
    "o3dmi_sample_index": (_i64, [C.c_uint64, _i64, _i64]),
    "o3dmi_pointcloud_random_sample_indices": (
        _i32, [_i64, _d, C.c_uint64, _vp, C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_aabb_mask": (
        _i32, [_vp, _i64, _i32, _dp, _dp, _vp, C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_obb_mask": (
        _i32, [_vp, _i64, _i32, _dp, _dp, _dp, _vp, C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_min_max_bound": (_i32, [_vp, _i64, _i32, _dp, _dp,
                                              _vp]),
    "o3dmi_pointcloud_nearest_distance": (
        _i32, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp]),
    "o3dmi_metrics_from_sums": (
        _i32, [_i64, _i64, _dp, _dp, C.POINTER(_i64), _i32, C.POINTER(_i32),
               _i32, C.POINTER(_f), _i64]),
    "o3dmi_pointcloud_compute_metrics": (
        _i32, [_vp, _i64, _vp, _i64, _i32, C.POINTER(_i32), _i32,
               C.POINTER(_f), _i32, C.POINTER(_f), _i64,
               C.POINTER(MetricsRawC), _vp]),
    "o3dmi_pointcloud_smooth_laplacian": (
        _i32, [_vp, _i64, _i32, _i64, _d, _i32, _i32, _vp, _vp]),
    "o3dmi_pointcloud_smooth_taubin": (
        _i32, [_vp, _i64, _i32, _i64, _d, _d, _i32, _i32, _vp, _vp]),
    "o3dmi_pointcloud_smooth_mls": (
        _i32, [_vp, _vp, _i64, _i32, _d, _i32, _vp, _vp, _vp]),
    "o3dmi_pointcloud_smooth_bilateral": (
        _i32, [_vp, _vp, _i64, _i32, _d, _i32, _d, _d, _vp, _vp]),
    "o3dmi_pointcloud_compute_boundary_points": (
        _i32, [_vp, _vp, _i64, _i32, _d, _i32, _d, _vp, C.POINTER(_i64),
               _vp]),
    "o3dmi_pointcloud_boundary_from_neighbors": (
        _i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _d, _vp, _vp]),
    "o3dmi_pointcloud_normalize_normals": (_i32, [_vp, _i64, _i32, _vp]),
    "o3dmi_pointcloud_orient_normals_to_align_with_direction": (
        _i32, [_vp, _i64, _i32, _dp, _vp]),
    "o3dmi_pointcloud_orient_normals_towards_camera_location": (
        _i32, [_vp, _vp, _i64, _i32, _dp, _vp]),
    "o3dmi_slac_preprocess_point_cloud": (
        _i32, [_vp, _vp, _i64, _i32, _d, _i32, _vp, _vp, C.POINTER(_i64),
               _vp]),
    "o3dmi_vbg_to_device": (_i32, [_vp, _i32, C.POINTER(_vp)]),
    "o3dmi_hash_to_device": (_i32, [_vp, _i32, C.POINTER(_vp)]),
    "o3dmi_vbg_create": (_i32, [_i32, C.POINTER(C.c_char_p), C.POINTER(_i32),
                                C.POINTER(_i32), _f, _i64, _i64, _vp,
                                C.POINTER(_vp)]),
    "o3dmi_vbg_destroy": (_i32, [_vp]),
    "o3dmi_vbg_hashmap": (_vp, [_vp]),
    "o3dmi_vbg_set_block_ownership": (_i32, [_vp, _i32, _i32]),
    "o3dmi_vbg_attribute": (_vp, [_vp, C.c_char_p, C.POINTER(_i32),
                                  C.POINTER(_i32)]),
    "o3dmi_vbg_get_unique_block_coordinates": (
        _i32, [_vp, _vp, _i32, _i32, _i32, _dp, _dp, _f, _f, _f, _vp,
               C.POINTER(_i64), _vp]),
    "o3dmi_vbg_get_unique_block_coordinates_pcd": (
        _i32, [_vp, _vp, _i64, _f, _vp, _i64, C.POINTER(_i64), _vp]),
    "o3dmi_vbg_get_voxel_indices": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "o3dmi_vbg_get_voxel_coordinates": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "o3dmi_vbg_get_voxel_coordinates_and_flattened_indices": (
        _i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "o3dmi_vbg_integrate_blocks": (
        _i32, [_vp, _vp, _i64, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _dp,
               _dp, _dp, _f, _f, _f, _vp]),
    "o3dmi_vbg_integrate_frame": (
        _i32, [_vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _dp, _dp, _dp, _f,
               _f, _f, _vp]),
    "o3dmi_vbg_integrate_frames": (
        _i32, [_vp, _i32, C.POINTER(_vp), _i32, _i32, C.POINTER(_vp), _i32,
               _i32, _i32, _dp, _dp, _dp, _f, _f, _f, _i32, _vp]),
    "o3dmi_vbg_slice_chunk_frames": (_i32, [_i32]),
    "o3dmi_vbg_set_slice_capacity": (_i32, [_vp, _i32, _i32]),
    "o3dmi_vbg_slice_segment_bytes": (_i64, [_vp]),
    "o3dmi_vbg_touch_slice": (
        _i32, [_vp, _i32, C.POINTER(_vp), _i32, _i32, _dp, _dp, _f, _f, _f,
               _i32, _i32, _i32, _vp, _vp]),
    "o3dmi_vbg_integrate_frames_sliced": (
        _i32, [_vp, _i32, C.POINTER(_vp), _i32, _i32, C.POINTER(_vp), _i32,
               _i32, _i32, _dp, _dp, _dp, _f, _f, _f, _i32, C.POINTER(_vp),
               _vp]),
    "o3dmi_vbg_sliced_stats": (_i32, [_vp, C.POINTER(_i64), C.POINTER(_i64),
                                      C.POINTER(_i32), C.POINTER(_i32)]),
    "o3dmi_vbg_profile_begin": (_i32, [_vp, _i32, _i32]),
    "o3dmi_vbg_profile_end": (_i32, [_vp, _vp, C.POINTER(_d), C.POINTER(_i64),
                                     C.POINTER(_i64), C.POINTER(_i64)]),
    "o3dmi_rgbd_odometry_multiscale": (
        _i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _dp,
               _dp, _f, _f, _i32, C.POINTER(OdometryCriteriaC), _i32, _f, _f,
               _f,
               C.POINTER(OdometryResultC), _vp]),
    "o3dmi_rgbd_odometry_information_matrix": (
        _i32, [_vp, _vp, _i32, _i32, _i32, _dp, _dp, _f, _f, _f, _dp, _vp]),
    "o3dmi_vbg_last_frame_block_coordinates": (_i32, [_vp, _vp, _i64, _vp,
                                                       _vp]),
    "o3dmi_vbg_ray_cast_dev": (
        _i32, [_vp, _vp, _i64, _vp, _dp, _dp, _i32, _i32, _vp] + [_vp] * 10 +
        [_f, _f, _f, _f, _f, _i32, _vp]),
    "o3dmi_vbg_extract_point_cloud": (_i32, [_vp, _f, _i64, _vp, _vp, _vp,
                                             C.POINTER(_i64), _vp]),
    "o3dmi_vbg_extract_triangle_mesh": (_i32, [_vp, _f, _i64, _vp, _vp, _vp,
                                               _vp, C.POINTER(_i64),
                                               C.POINTER(_i64), _vp]),
    "o3dmi_slam_model_create": (_i32, [_f, _i32, _i64, _dp, _vp,
                                       C.POINTER(_vp)]),
    "o3dmi_slam_model_destroy": (_i32, [_vp]),
    "o3dmi_slam_model_voxel_grid": (_vp, [_vp]),
    "o3dmi_slam_model_get_current_frame_pose": (_i32, [_vp, _dp]),
    "o3dmi_slam_model_update_frame_pose": (_i32, [_vp, _i32, _dp]),
    "o3dmi_slam_model_frame_id": (_i32, [_vp]),
    "o3dmi_slam_model_synthesize_model_frame": (
        _i32, [_vp, _dp, _i32, _i32, _f, _f, _f, _f, _f, _vp, _vp, _vp]),
    "o3dmi_slam_model_track_frame_to_model": (
        _i32, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _dp, _f, _f,
               _f, _i32, _i32, C.POINTER(OdometryCriteriaC),
               C.POINTER(OdometryResultC), _vp]),
    "o3dmi_slam_model_integrate": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32,
                                          _dp, _f, _f, _f, _vp]),
    "o3dmi_slam_model_frustum_block_count": (_i64, [_vp]),
    "o3dmi_slam_model_frustum_block_coords": (_vp, [_vp]),
    "o3dmi_slam_model_extract_point_cloud": (_i32, [_vp, _f, _i64, _vp, _vp,
                                                    _vp, C.POINTER(_i64),
                                                    _vp]),
    "o3dmi_slam_model_extract_triangle_mesh": (
        _i32, [_vp, _f, _i64, _vp, _vp, _vp, _vp, C.POINTER(_i64),
               C.POINTER(_i64), _vp]),
    "o3dmi_npz_create": (_i32, [C.POINTER(_vp)]),
    "o3dmi_npz_destroy": (_i32, [_vp]),
    "o3dmi_npz_add": (_i32, [_vp, C.c_char_p, _i32, _i32, C.POINTER(_i64),
                             _vp]),
    "o3dmi_npz_count": (_i32, [_vp]),
    "o3dmi_npz_name": (C.c_char_p, [_vp, _i32]),
    "o3dmi_npz_get": (_i32, [_vp, C.c_char_p, C.POINTER(_i32),
                             C.POINTER(_i32), C.POINTER(_i64),
                             C.POINTER(_vp)]),
    "o3dmi_npz_write": (_i32, [_vp, C.c_char_p]),
    "o3dmi_npz_read": (_i32, [C.c_char_p, C.POINTER(_vp)]),
    "o3dmi_vbg_export_blocks": (_i32, [_vp, _i64, _vp, C.POINTER(_vp),
                                       C.POINTER(_i64), _vp]),
    "o3dmi_vbg_merge_blocks": (_i32, [_vp, _vp, C.POINTER(_vp), _i64, _vp]),
    "o3dmi_vbg_save": (_i32, [_vp, C.c_char_p, _vp]),
    "o3dmi_vbg_load": (_i32, [C.c_char_p, _vp, C.POINTER(_vp)]),
    "o3dmi_vbg_attribute_count": (_i32, [_vp]),
    "o3dmi_vbg_attribute_name": (C.c_char_p, [_vp, _i32]),
    "o3dmi_vbg_voxel_size": (_f, [_vp]),
    "o3dmi_vbg_block_resolution": (_i64, [_vp]),
    "o3dmi_vbg_ray_cast": (
        _i32, [_vp, _vp, _i64, _dp, _dp, _i32, _i32, _vp] + [_vp] * 10 +
        [_f, _f, _f, _f, _f, _i32, _vp]),
    "o3dmi_vbg_ray_cast_sharded": (
        _i32, [_vp, _vp, _i64, _dp, _dp, _i32, _i32, _vp] + [_vp] * 4 +
        [_f, _f, _f, _f, _f, _i32, _vp]),
    "o3dmi_vbg_profile_distinct_blocks": (_i64, [_vp]),
    "o3dmi_vbg_division_forms": (_i32, [_f, _f, _i32]),
    "o3dmi_vbg_step_form_launches": (_i64, [_i32]),
    "o3dmi_vbg_front_tile_key_limit": (_i32, []),
    "o3dmi_vbg_profile_launches": (_i64, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "o3dmi_rccl_available": (_i32, []),
    "o3dmi_rccl_unique_id": (_i32, [_vp]),
    "o3dmi_comm_create_rccl": (_i32, [_vp, _i32, _i32, C.POINTER(_vp)]),
    "o3dmi_comm_adopt_rccl": (_i32, [_vp, C.POINTER(_vp)]),
    "o3dmi_comm_create_custom": (_i32, [_vp, _vp, _i32, _i32,
                                        C.POINTER(_vp)]),
    "o3dmi_comm_destroy": (_i32, [_vp]),
    "o3dmi_comm_rank": (_i32, [_vp]),
    "o3dmi_preload": (_i32, []),
    "o3dmi_comm_world": (_i32, [_vp]),
    "o3dmi_comm_rccl_ranks": (_i32, [_vp]),
    "o3dmi_set_comm": (_i32, [_vp]),
    "o3dmi_set_rccl_comm": (_i32, [_vp]),
    "o3dmi_comm_allreduce_sum_f64": (_i32, [_vp, _vp, _i64, _vp]),
    "o3dmi_comm_allgather": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "o3dmi_comm_alltoallv": (_i32, [_vp, _vp, C.POINTER(_i64),
                                    C.POINTER(_i64), _vp, C.POINTER(_i64),
                                    C.POINTER(_i64), _vp]),
    "o3dmi_vbg_merge_frame_sharded": (_i32, [_vp, _vp, _vp]),
    "o3dmi_vbg_allgather_owned_blocks": (_i32, [_vp, _vp, _vp]),
    # include/o3d_mi355x.h
    "o3dmi_sort_pairs_u32": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    # TriangleMesh operators: (positions, v, dtype, triangles, m, index_dtype,
    # ...) wherever a call takes positions
    "o3dmi_trianglemesh_compute_triangle_normals": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp]),
    "o3dmi_trianglemesh_compute_triangle_areas": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp]),
    "o3dmi_trianglemesh_surface_area": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _dp, _vp]),
    "o3dmi_trianglemesh_normalize_normals": (_i32, [_vp, _i64, _i32, _vp]),
    "o3dmi_trianglemesh_compute_vertex_normals": (
        _i32, [_vp, _i64, _i32, _vp, _i32, _i64, _vp, _vp]),
    "o3dmi_trianglemesh_vertex_normals": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp, _i32, _vp]),
    "o3dmi_trianglemesh_get_non_manifold_edges": (
        _i32, [_vp, _i64, _i32, _i64, _i32, _vp, _i64, C.POINTER(_i64), _vp]),
    "o3dmi_trianglemesh_cluster_connected_triangles": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, C.POINTER(_i64), _vp,
               _vp, _i64, _vp]),
    "o3dmi_trianglemesh_select_faces_by_mask": (
        _i32, [_vp, _i64, _i32, _i64, _vp, _vp, _vp, C.POINTER(_i64),
               C.POINTER(_i64), _vp]),
    "o3dmi_trianglemesh_select_by_index": (
        _i32, [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _vp, _vp,
               C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "o3dmi_trianglemesh_remove_unreferenced_vertices": (
        _i32, [_vp, _i64, _i32, _i64, _vp, _vp, C.POINTER(_i64), _vp]),
    "o3dmi_trianglemesh_remove_duplicated_vertices": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp, C.POINTER(_i64),
               _vp]),
    "o3dmi_trianglemesh_remove_duplicated_triangles": (
        _i32, [_vp, _i64, _i32, _i64, _vp, _vp, C.POINTER(_i64), _vp]),
    "o3dmi_trianglemesh_remove_degenerate_triangles": (
        _i32, [_vp, _i64, _i32, _i64, _vp, _vp, C.POINTER(_i64), _vp]),
    "o3dmi_trianglemesh_compute_adjacency_list": (
        _i32, [_vp, _i64, _i32, _i64, _vp, _vp, _i64, C.POINTER(_i64), _vp]),
    # (positions, v, dtype, normals, colors, attr_dtype, triangles, m,
    # index_dtype, iterations, ...)
    "o3dmi_trianglemesh_filter_sharpen": (
        _i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _d,
               _i32, _vp, _vp, _vp, _vp]),
    "o3dmi_trianglemesh_filter_smooth_simple": (
        _i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _i32,
               _vp, _vp, _vp, _vp]),
    "o3dmi_trianglemesh_filter_smooth_laplacian": (
        _i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _d,
               _i32, _vp, _vp, _vp, _vp]),
    "o3dmi_trianglemesh_filter_smooth_taubin": (
        _i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _d, _d,
               _i32, _vp, _vp, _vp, _vp]),
    "o3dmi_trianglemesh_simplify_vertex_clustering": (
        _i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _i32, _d, _i32,
               _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), _vp]),
    # (..., index_dtype, number_of_iterations, positions_out, normals_out,
    # colors_out, vertex_capacity, triangles_out, n_vertices, n_triangles)
    "o3dmi_trianglemesh_subdivide_midpoint": (
        _i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _vp,
               _vp, _vp, _i64, _vp, C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "o3dmi_trianglemesh_subdivide_loop": (
        _i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _vp,
               _vp, _vp, _i64, _vp, C.POINTER(_i64), C.POINTER(_i64), _vp]),
    # (..., index_dtype, point, normal, positions_out, normals_out,
    # colors_out, vertex_capacity, triangles_out, triangle_capacity,
    # triangle_source, vertex_source, vertex_t, n_vertices, n_triangles)
    "o3dmi_trianglemesh_clip_plane": (
        _i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _i32, _dp, _dp,
               _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
               C.POINTER(_i64), C.POINTER(_i64), _vp]),
    # (..., index_dtype, point, normal, contour_values, n_contours,
    # points_out, normals_out, colors_out, point_capacity, lines_out,
    # line_capacity, line_triangle, line_contour, point_source, point_t,
    # n_points, n_lines)
    "o3dmi_trianglemesh_slice_plane": (
        _i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i64, _i32, _dp, _dp,
               _dp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp,
               C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "o3dmi_mesh_sample_draw": (
        _i32, [C.c_uint64, _i64, _dp, C.POINTER(_f), C.POINTER(_f)]),
    "o3dmi_trianglemesh_sample_points_uniformly": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _i64, C.c_uint64, _vp, _vp,
               _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "o3dmi_mesh_bvh_create": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, C.POINTER(_vp), _vp]),
    "o3dmi_mesh_bvh_destroy": (_i32, [_vp]),
    "o3dmi_mesh_bvh_closest_points": (
        _i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "o3dmi_trianglemesh_closest_points": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _vp,
               _vp, _vp, _vp]),
    "o3dmi_trianglemesh_compute_distance": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _vp, _vp]),
    "o3dmi_trianglemesh_compute_metrics": (
        _i32, [_vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _i32, _i32,
               C.POINTER(_i32), _i32, C.POINTER(_f), _i32, _i64, C.c_uint64,
               C.POINTER(_f), _i64, C.POINTER(MetricsRawC), _vp]),
    # ray queries: (handle, rays, q, dtype, ...)
    "o3dmi_mesh_bvh_cast_rays": (
        _i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "o3dmi_mesh_bvh_test_occlusions": (
        _i32, [_vp, _vp, _i64, _i32, _f, _f, _vp, _vp]),
    "o3dmi_mesh_bvh_count_intersections": (
        _i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "o3dmi_mesh_bvh_list_intersections": (
        _i32, [_vp, _vp, _i64, _i32, _vp, _i64, C.POINTER(_i64), _vp, _vp,
               _vp, _vp, _vp, _vp]),
    "o3dmi_raycast_vote_directions": (_i32, [_i32, C.POINTER(_f)]),
    "o3dmi_mesh_bvh_compute_occupancy": (
        _i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "o3dmi_mesh_bvh_compute_signed_distance": (
        _i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "o3dmi_create_rays_pinhole": (_i32, [_dp, _dp, _i32, _i32, _vp, _vp]),
    "o3dmi_trianglemesh_cast_rays": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _vp,
               _vp, _vp, _vp]),
    "o3dmi_trianglemesh_compute_signed_distance": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp]),
    # topology and intersection queries: (triangles, m, index dtype, v, ...)
    # or (positions, v, dtype, triangles, m, index dtype, ...)
    "o3dmi_trianglemesh_euler_poincare_characteristic": (
        _i32, [_vp, _i64, _i32, _i64, C.POINTER(_i64), _vp]),
    "o3dmi_trianglemesh_is_edge_manifold": (
        _i32, [_vp, _i64, _i32, _i64, _i32, C.POINTER(_i32), _vp]),
    "o3dmi_trianglemesh_get_non_manifold_vertices": (
        _i32, [_vp, _i64, _i32, _i64, _vp, _i64, C.POINTER(_i64), _vp]),
    "o3dmi_trianglemesh_orient_triangles": (
        _i32, [_vp, _i64, _i32, _i64, _vp, C.POINTER(_i32), _vp]),
    "o3dmi_trianglemesh_get_self_intersecting_triangles": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, C.POINTER(_i64),
               _vp]),
    "o3dmi_trianglemesh_is_self_intersecting": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, C.POINTER(_i32), _vp]),
    "o3dmi_trianglemesh_is_intersecting": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64,
               _i32, C.POINTER(_i32), _vp]),
    "o3dmi_trianglemesh_is_watertight": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, C.POINTER(_i32), _vp]),
    "o3dmi_trianglemesh_get_volume": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _dp, _vp]),
    # (points, n, dtype, [camera_location, radius,] positions_out,
    # point_indices_out, vertex_capacity, triangles_out, triangle_capacity,
    # index_dtype, n_vertices, n_triangles, stream)
    "o3dmi_pointcloud_convex_hull": (
        _i32, [_vp, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _i32,
               C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "o3dmi_pointcloud_hidden_point_removal": (
        _i32, [_vp, _i64, _i32, _dp, _d, _vp, _vp, _i64, _vp, _i64, _i32,
               C.POINTER(_i64), C.POINTER(_i64), _vp]),
    # (points, n, dtype, method, center[3], rotation[9], extent[3], stream)
    "o3dmi_pointcloud_oriented_bounding_box": (
        _i32, [_vp, _i64, _i32, _i32, _dp, _dp, _dp, _vp]),
    # (points, n, dtype, center[3], rotation[9], radii[3], iterations, stream)
    "o3dmi_pointcloud_oriented_bounding_ellipsoid": (
        _i32, [_vp, _i64, _i32, _dp, _dp, _dp, C.POINTER(_i32), _vp]),
    # host-only: (n, sums[9], mean[3], rotation[9])
    "o3dmi_bounding_box_frame_from_moments": (_i32, [_i64, _dp, _dp, _dp]),
    # host-only: (sums[9], center[3], rotation[9], radii[3])
    "o3dmi_bounding_ellipsoid_from_moments": (_i32, [_dp, _dp, _dp, _dp]),
})

# o3dmi_transport_t (include/o3d_mi355x_host.h): the caller-provided collectives
TRANSPORT_ALLREDUCE = C.CFUNCTYPE(_i32, _vp, _vp, _i64, _vp)
TRANSPORT_ALLGATHER = C.CFUNCTYPE(_i32, _vp, _vp, _vp, _i64, _vp)
TRANSPORT_ALLTOALLV = C.CFUNCTYPE(_i32, _vp, _vp, C.POINTER(_i64),
                                  C.POINTER(_i64), _vp, C.POINTER(_i64),
                                  C.POINTER(_i64), _vp)


class TransportC(C.Structure):
    _fields_ = [("allreduce_sum_f64", TRANSPORT_ALLREDUCE),
                ("allgather", TRANSPORT_ALLGATHER),
                ("alltoallv", TRANSPORT_ALLTOALLV)]

# Exported entry points that are in no public header (declared in csrc/*.h):
# bound here, once, for the tests and tools that drive them.
INTERNAL_PROTOTYPES = {
    # csrc/pointcloud_smooth.h: (kind, points, normals, indices, dist2, counts,
    # n, width, dtype, p0, p1, out_points, out_normals, mask, stream)
    "o3dmi_internal_pointcloud_smooth_from_neighbors": (
        _i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _d, _d, _vp,
               _vp, _vp, _vp]),
    # csrc/nns.h: (index, queries, ids, nq, max_knn, idx, dist2, counts,
    # stream)
    "o3dmi_internal_nns_hybrid_search_wide": (
        _i32, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    # csrc/mesh_bvh.h: (handle, queries, q, points, ids, uvs, normals,
    # distance, sort_queries, visits[2], stream)
    "o3dmi_internal_mesh_bvh_query": (
        _i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32,
               C.POINTER(C.c_uint64), _vp]),
    # csrc/mesh_bvh.h: (handle, kind, rays, q, tnear, tfar, t_hit,
    # geometry_ids, primitive_ids, uvs, normals, occluded, counts, sort_rays,
    # visits[2], stream)
    "o3dmi_internal_mesh_bvh_ray_query": (
        _i32, [_vp, _i32, _vp, _i64, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp,
               _vp, _i32, C.POINTER(C.c_uint64), _vp]),
    # csrc/trianglemesh_topology.h: (positions, v, dtype, triangles, m, index
    # dtype, kind, n, visits[2], stream)
    "o3dmi_internal_trianglemesh_self_intersections": (
        _i32, [_vp, _i64, _i32, _vp, _i64, _i32, _i32, C.POINTER(_i64),
               C.POINTER(C.c_uint64), _vp]),
    # csrc/pointcloud_hull.h: {rounds, sweep rounds, winners, refused} of the
    # thread's last hull call
    "o3dmi_internal_pointcloud_hull_stats": (_i32, [C.POINTER(_i64)]),
    # csrc/bounding_volume.h: the resident form's capacity; {hull vertices,
    # hull triangles, iterations, form, winner} and 16 values of the thread's
    # last bounding-volume call
    # o3dmi_pointcloud_oriented_bounding_box's MINIMAL_APPROX with (split) in
    # the place of (method)
    "o3dmi_internal_pointcloud_obb_minimal_approx": (
        _i32, [_vp, _i64, _i32, _i32, _dp, _dp, _dp, _vp]),
    "o3dmi_internal_obe_resident_capacity": (_i64, []),
    "o3dmi_internal_bounding_volume_stats": (
        _i32, [C.POINTER(_i64), _dp]),
    # csrc/fgr.h: o3dmi_fgr_tuple_test with (first_batch) before the outputs
    # and (n_batches) after them
    "o3dmi_internal_fgr_tuple_test": (
        _i32, [C.c_uint64, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _d, _i64,
               _i64, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64),
               _vp]),
    # csrc/fgr.h: o3dmi_fgr_optimize with (form) before scratch and
    # (form_out) after out
    "o3dmi_internal_fgr_optimize": (
        _i32, [_vp, _i64, _vp, _i64, _vp, _i64, _d, _d, _i32, _d, _i32, _i32,
               _vp, _vp, C.POINTER(_i32), _vp]),
    "o3dmi_internal_fgr_stream_scratch_bytes": (C.c_size_t, [_i64]),
    "o3dmi_internal_fgr_resident_capacity": (_i64, []),
    # csrc/feature.h: (a, na, b, nb, dim, dtype, nn, stream)
    "o3dmi_internal_feature_nn1": (
        _i32, [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp]),
}

_lib = None


class O3DMIError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        msg = lib().o3dmi_status_string(status).decode()
        detail = lib().o3dmi_last_error().decode()
        super().__init__("%s failed: %s (%s)" % (where, msg, detail))


def lib():
    """Loads the HIP library; raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                "open3d_amd: %s not found -- the HIP extension is mandatory "
                "(run `python -m open3d_amd.build`); there is no CPU "
                "fallback." % SO_PATH)
        # torch first: it ships its own HIP runtime, and the process must end
        # up with ONE libamdhip64 (the first one loaded wins the soname). With
        # the order reversed the second runtime sees no device.
        import torch  # noqa: F401
        L = C.CDLL(SO_PATH)
        for name, (res, args) in list(PROTOTYPES.items()) + \
                list(INTERNAL_PROTOTYPES.items()):
            fn = getattr(L, name)  # AttributeError if a symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, where):
    if status != OK:
        raise O3DMIError(status, where)


def ptr(t):
    """Device (or host) pointer of a torch tensor / None."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def f64p(a):
    """numpy float64 contiguous array -> double*."""
    return a.ctypes.data_as(_dp)
