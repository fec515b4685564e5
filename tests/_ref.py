"""ctypes binding of oracle/_ref/libo3d_ref.so -- TEST INFRASTRUCTURE ONLY.

libo3d_ref.so holds the reference's OWN hot-path kernel files
(VoxelBlockGridCPU.cpp + VoxelBlockGridImpl.h, RegistrationCPU.cpp,
TransformationConverter.cpp, TransformImpl.h, PointCloudCPU.cpp,
FeatureCPU.cpp + FeatureImpl.h, FillInLinearSystemCPU.cpp +
FillInLinearSystemImpl.h ...) compiled
from /root/reference through the stand-in headers in oracle/ref_shim
(`make -C oracle ref`). It exists only where /root/reference exists (this build
container) or where a prebuilt copy travelled with the tree (the GPU box).
`available()` says whether it can be used; tests skip otherwise.

Function names and argument order mirror tests/_oracle.py (and, for FPFH,
Doppler ICP and the SLAC fill-ins, tests/_fpfh_oracle.py,
tests/_doppler_oracle.py, tests/_slac_oracle.py and
tests/_slac_nonrigid_oracle.py) so the same inputs can be run through both.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE_DIR = os.path.join(_ROOT, "oracle")
_SO = os.path.join(_ORACLE_DIR, "_ref", "libo3d_ref.so")
_REFERENCE = "/root/reference/cpp/open3d"

_lib = None
c_vp = C.c_void_p


def available():
    if os.path.exists(_SO):
        return True
    if os.path.isdir(_REFERENCE):
        try:
            subprocess.check_call(["make", "-s", "-C", _ORACLE_DIR, "ref"])
        except Exception:
            return False
        return os.path.exists(_SO)
    return False


def lib():
    global _lib
    if _lib is None:
        if not available():
            raise RuntimeError("oracle/_ref/libo3d_ref.so is not available")
        _lib = C.CDLL(_SO)
        L = _lib
        L.ref_last_error.restype = C.c_char_p
        L.ref_depth_touch.restype = C.c_int64
        L.ref_pointcloud_touch.restype = C.c_int64
        L.ref_unproject.restype = C.c_int64
        L.ref_robust_weight.restype = C.c_double
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(c_vp)


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _check(st, what):
    if st != 0:
        raise RuntimeError("%s: %s" % (what, lib().ref_last_error().decode()))


def set_threads(n):
    lib().ref_set_threads(int(n))


def set_reduce_schedule(seed, min_chunk=1024):
    """Schedule of the stand-in tbb::parallel_reduce: seed 0 = one sequential
    chunk; otherwise seeded random splits down to <= min_chunk elements."""
    lib().ref_set_reduce_schedule(C.c_ulonglong(int(seed)),
                                  C.c_longlong(int(min_chunk)))


def p2plane_accumulate_address():
    """Address of ref_p2plane_accumulate (for orc.set_p2plane_hook)."""
    return C.cast(lib().ref_p2plane_accumulate, C.c_void_p).value


def depth_touch(depth, K, T, resolution, voxel_size, sdf_trunc, depth_scale,
                depth_max, stride=4):
    depth = np.ascontiguousarray(depth)
    rows, cols = depth.shape[:2]
    cap = (rows // stride) * (cols // stride) * 4 + 16
    out = np.zeros((cap, 3), np.int32)
    K, T = _f64(K), _f64(T)
    n = lib().ref_depth_touch(_p(depth), int(depth.dtype == np.float32), rows,
                              cols, _p(K), _p(T), int(resolution),
                              C.c_float(voxel_size), C.c_float(sdf_trunc),
                              C.c_float(depth_scale), C.c_float(depth_max),
                              int(stride), _p(out), C.c_int64(cap))
    if n < 0:
        raise RuntimeError(lib().ref_last_error().decode())
    return out[:n].copy()


def pointcloud_touch(points, resolution, voxel_size, sdf_trunc):
    points = np.ascontiguousarray(points, dtype=np.float32)
    n = points.shape[0]
    cap = n * 27 + 16
    out = np.zeros((cap, 3), np.int32)
    m = lib().ref_pointcloud_touch(_p(points), C.c_int64(n), int(resolution),
                                   C.c_float(voxel_size), C.c_float(sdf_trunc),
                                   _p(out), C.c_int64(cap))
    if m < 0:
        raise RuntimeError(lib().ref_last_error().decode())
    return out[:m].copy()


def voxel_coords_flat(buf_indices, block_keys, resolution, voxel_size):
    buf_indices = np.ascontiguousarray(buf_indices, dtype=np.int32)
    block_keys = np.ascontiguousarray(block_keys, dtype=np.int32)
    n = buf_indices.shape[0] * resolution ** 3
    coords = np.zeros((n, 3), np.float32)
    flat = np.zeros(n, np.int64)
    _check(lib().ref_voxel_coords_flat(
        _p(buf_indices), C.c_int64(buf_indices.shape[0]), _p(block_keys),
        C.c_int64(block_keys.shape[0]), int(resolution), C.c_float(voxel_size),
        _p(coords), _p(flat)), "ref_voxel_coords_flat")
    return coords, flat


def integrate(depth, color, indices, block_keys, tsdf, weight, color_buf, K_d,
              K_c, T, resolution, voxel_size, sdf_trunc, depth_scale,
              depth_max):
    """In place on tsdf / weight / color_buf."""
    depth = np.ascontiguousarray(depth)
    input_is_f32 = int(depth.dtype == np.float32)
    grid_is_f32 = int(weight.dtype == np.float32)
    if color is not None and color.size > 0:
        color = np.ascontiguousarray(color)
        crow, ccol = color.shape[:2]
    else:
        color, crow, ccol = None, 0, 0
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    block_keys = np.ascontiguousarray(block_keys, dtype=np.int32)
    K_d, K_c, T = _f64(K_d), _f64(K_c), _f64(T)
    _check(lib().ref_integrate(
        _p(depth), depth.shape[0], depth.shape[1], _p(color), crow, ccol,
        input_is_f32, _p(indices), C.c_int64(indices.shape[0]), _p(block_keys),
        C.c_int64(tsdf.shape[0]), _p(tsdf), _p(weight), _p(color_buf),
        grid_is_f32, _p(K_d), _p(K_c), _p(T), int(resolution),
        C.c_float(voxel_size), C.c_float(sdf_trunc), C.c_float(depth_scale),
        C.c_float(depth_max)), "ref_integrate")


def estimate_range(block_keys, K, T, h, w, down_factor, block_resolution,
                   voxel_size, depth_min, depth_max, frag_buffer_size=0):
    block_keys = np.ascontiguousarray(block_keys, dtype=np.int32)
    out = np.zeros((h // down_factor, w // down_factor, 2), np.float32)
    K, T = _f64(K), _f64(T)
    _check(lib().ref_estimate_range(
        _p(block_keys), C.c_int64(block_keys.shape[0]), _p(out), _p(K), _p(T),
        int(h), int(w), int(down_factor), C.c_int64(block_resolution),
        C.c_float(voxel_size), C.c_float(depth_min), C.c_float(depth_max),
        int(frag_buffer_size)), "ref_estimate_range")
    return out


def raycast(hash_keys, hash_buf_indices, tsdf, weight, color_buf, range_map, K,
            T, h, w, block_resolution, voxel_size, depth_scale, depth_min,
            depth_max, weight_threshold, trunc_voxel_multiplier,
            range_map_down_factor, attrs=("depth", "color")):
    grid_is_f32 = int(weight.dtype == np.float32)
    K, T = _f64(K), _f64(T)
    shapes = {"depth": (1, np.float32), "vertex": (3, np.float32),
              "color": (3, np.float32), "normal": (3, np.float32),
              "index": (8, np.int64), "mask": (8, np.uint8),
              "interp_ratio": (8, np.float32),
              "interp_ratio_dx": (8, np.float32),
              "interp_ratio_dy": (8, np.float32),
              "interp_ratio_dz": (8, np.float32)}
    out = {}
    for a in attrs:
        c, dt = shapes[a]
        out[a] = np.full((h, w, c), 77, dt)
    g = lambda a: _p(out[a]) if a in out else None
    hash_keys = np.ascontiguousarray(hash_keys, dtype=np.int32)
    hash_buf_indices = np.ascontiguousarray(hash_buf_indices, dtype=np.int32)
    range_map = np.ascontiguousarray(range_map, dtype=np.float32)
    _check(lib().ref_raycast(
        _p(hash_keys), _p(hash_buf_indices), C.c_int64(hash_keys.shape[0]),
        C.c_int64(tsdf.shape[0]), _p(tsdf), _p(weight), _p(color_buf),
        grid_is_f32, _p(range_map), g("depth"), g("vertex"), g("color"),
        g("normal"), g("index"), g("mask"), g("interp_ratio"),
        g("interp_ratio_dx"), g("interp_ratio_dy"), g("interp_ratio_dz"),
        _p(K), _p(T), int(h), int(w), int(block_resolution),
        C.c_float(voxel_size), C.c_float(depth_scale), C.c_float(depth_min),
        C.c_float(depth_max), C.c_float(weight_threshold),
        C.c_float(trunc_voxel_multiplier), int(range_map_down_factor)),
        "ref_raycast")
    if "mask" in out:
        out["mask"] = out["mask"].astype(bool)
    return out


def unproject(depth, colors_f32, K, T, depth_scale, depth_max, stride=1):
    depth = np.ascontiguousarray(depth)
    rows, cols = depth.shape[:2]
    n = (rows // stride) * (cols // stride)
    pts = np.zeros((n, 3), np.float32)
    cols_out = None
    if colors_f32 is not None:
        colors_f32 = np.ascontiguousarray(colors_f32, dtype=np.float32)
        cols_out = np.zeros((n, 3), np.float32)
    K, T = _f64(K), _f64(T)
    m = lib().ref_unproject(_p(depth), int(depth.dtype == np.float32), rows,
                            cols, _p(colors_f32), _p(pts), _p(cols_out), _p(K),
                            _p(T), C.c_float(depth_scale),
                            C.c_float(depth_max), C.c_int64(stride))
    if m < 0:
        raise RuntimeError(lib().ref_last_error().decode())
    if cols_out is None:
        return pts[:m].copy(), None
    return pts[:m].copy(), cols_out[:m].copy()


def robust_weight(method, scaling, shape, residual, f64=False):
    return float(lib().ref_robust_weight(int(f64), int(method),
                                         C.c_double(scaling),
                                         C.c_double(shape),
                                         C.c_double(residual)))


def p2plane_accumulate(src, tgt, tgt_n, corr, method=0, scaling=1.0,
                       shape=1.0):
    """29 sums accumulated in the point dtype (sequential order)."""
    src = np.ascontiguousarray(src)
    tgt = np.ascontiguousarray(tgt, dtype=src.dtype)
    tgt_n = np.ascontiguousarray(tgt_n, dtype=src.dtype)
    corr = np.ascontiguousarray(corr, dtype=np.int64).reshape(-1)
    out = np.zeros(29, np.float64)
    _check(lib().ref_p2plane_accumulate(
        _p(src), _p(tgt), _p(tgt_n), _p(corr), C.c_int64(src.shape[0]),
        int(src.dtype == np.float64), int(method), C.c_double(scaling),
        C.c_double(shape), _p(out)), "ref_p2plane_accumulate")
    return out


def symmetric_accumulate(src, tgt, sn, tn, corr, source_mean, target_mean,
                         method=0, scaling=1.0, shape=1.0):
    """ComputePoseSymmetricKernelCPU: 29 sums in the point dtype."""
    src = np.ascontiguousarray(src)
    dt = src.dtype
    tgt, sn, tn = (np.ascontiguousarray(a, dtype=dt) for a in (tgt, sn, tn))
    corr = np.ascontiguousarray(corr, dtype=np.int64).reshape(-1)
    out = np.zeros(29, np.float64)
    ms = np.ascontiguousarray(source_mean, dtype=np.float64)
    mt = np.ascontiguousarray(target_mean, dtype=np.float64)
    _check(lib().ref_symmetric_accumulate(
        _p(src), _p(tgt), _p(sn), _p(tn), _p(corr), C.c_int64(src.shape[0]),
        int(dt == np.float64), _p(ms), _p(mt), int(method),
        C.c_double(scaling), C.c_double(shape), _p(out)),
        "ref_symmetric_accumulate")
    return out


def colored_accumulate(src, src_c, tgt, tn, tc, tg, corr, lambda_geometric,
                       method=0, scaling=1.0, shape=1.0):
    """ComputePoseColoredICPKernelCPU: 29 sums in the point dtype."""
    src = np.ascontiguousarray(src)
    dt = src.dtype
    src_c, tgt, tn, tc, tg = (np.ascontiguousarray(a, dtype=dt)
                              for a in (src_c, tgt, tn, tc, tg))
    corr = np.ascontiguousarray(corr, dtype=np.int64).reshape(-1)
    out = np.zeros(29, np.float64)
    _check(lib().ref_colored_accumulate(
        _p(src), _p(src_c), _p(tgt), _p(tn), _p(tc), _p(tg), _p(corr),
        C.c_int64(src.shape[0]), int(dt == np.float64),
        C.c_double(lambda_geometric), int(method), C.c_double(scaling),
        C.c_double(shape), _p(out)), "ref_colored_accumulate")
    return out


def information_matrix(tgt, corr):
    """ComputeInformationMatrixCPU: GTG {6,6} float64."""
    tgt = np.ascontiguousarray(tgt)
    corr = np.ascontiguousarray(corr, dtype=np.int64).reshape(-1)
    G = np.zeros((6, 6), np.float64)
    _check(lib().ref_information_matrix(
        _p(tgt), _p(corr), C.c_int64(corr.shape[0]), C.c_int64(tgt.shape[0]),
        int(tgt.dtype == np.float64), _p(G)), "ref_information_matrix")
    return G


def p2point_sxy(src, tgt, corr):
    """Get3x3SxyLinearSystem (RegistrationCPU.cpp:495-617) in the point dtype:
    (Sxy {3,3}, source_mean {3}, target_mean {3}, inlier_count)."""
    src = np.ascontiguousarray(src)
    tgt = np.ascontiguousarray(tgt, dtype=src.dtype)
    corr = np.ascontiguousarray(corr, dtype=np.int64).reshape(-1)
    S = np.zeros((3, 3), np.float64)
    ms = np.zeros(3, np.float64)
    mt = np.zeros(3, np.float64)
    cnt = C.c_int(0)
    _check(lib().ref_p2point_sxy(
        _p(src), _p(tgt), _p(corr), C.c_int64(src.shape[0]),
        int(src.dtype == np.float64), _p(S), _p(ms), _p(mt), C.byref(cnt)),
        "ref_p2point_sxy")
    return S, ms, mt, cnt.value


def compute_pose_p2plane(src, tgt, tgt_n, corr, method=0, scaling=1.0,
                         shape=1.0):
    src = np.ascontiguousarray(src)
    tgt = np.ascontiguousarray(tgt, dtype=src.dtype)
    tgt_n = np.ascontiguousarray(tgt_n, dtype=src.dtype)
    corr = np.ascontiguousarray(corr, dtype=np.int64).reshape(-1)
    pose = np.zeros(6, np.float64)
    residual, count = C.c_float(0), C.c_int(0)
    _check(lib().ref_compute_pose_p2plane(
        _p(src), _p(tgt), _p(tgt_n), _p(corr), C.c_int64(src.shape[0]),
        C.c_int64(tgt.shape[0]), int(src.dtype == np.float64), int(method),
        C.c_double(scaling), C.c_double(shape), _p(pose), C.byref(residual),
        C.byref(count)), "ref_compute_pose_p2plane")
    return pose, residual.value, count.value


def decode_and_solve6x6(A29):
    A29 = _f64(A29)
    pose = np.zeros(6, np.float64)
    residual, count = C.c_float(0), C.c_int(0)
    st = lib().ref_decode_and_solve6x6(_p(A29), _p(pose), C.byref(residual),
                                       C.byref(count))
    return st, pose, residual.value, count.value


def pose_to_transformation(pose):
    pose = _f64(pose)
    T = np.zeros((4, 4), np.float64)
    _check(lib().ref_pose_to_transformation(_p(pose), _p(T)),
           "ref_pose_to_transformation")
    return T


def transform_points(T, pts):
    T = _f64(T)
    pts = np.array(pts, copy=True, order="C")
    _check(lib().ref_transform_points(_p(T), _p(pts), C.c_int64(pts.shape[0]),
                                      int(pts.dtype == np.float64)),
           "ref_transform_points")
    return pts


def transform_normals(T, nrm):
    T = _f64(T)
    nrm = np.array(nrm, copy=True, order="C")
    _check(lib().ref_transform_normals(_p(T), _p(nrm),
                                       C.c_int64(nrm.shape[0]),
                                       int(nrm.dtype == np.float64)),
           "ref_transform_normals")
    return nrm


# ---------------------------------------------------------------------------
# RGB-D odometry front end: ImageCPU.cpp / RGBDOdometryCPU.cpp bodies
# ---------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def clip_transform(src, scale, min_value, max_value, clip_fill):
    src = np.ascontiguousarray(src)
    rows, cols = src.shape[:2]
    dst = np.empty((rows, cols), np.float32)
    _check(lib().ref_clip_transform(_p(src), int(src.dtype == np.float32),
                                    C.c_int64(rows), C.c_int64(cols),
                                    C.c_float(scale), C.c_float(min_value),
                                    C.c_float(max_value), C.c_float(clip_fill),
                                    _p(dst)), "ClipTransformCPU")
    return dst


def pyrdown_depth(src, depth_diff, invalid_fill):
    src = _f32(src)
    rows, cols = src.shape[:2]
    dst = np.empty((rows // 2, cols // 2), np.float32)
    _check(lib().ref_pyrdown_depth(_p(src), rows, cols, C.c_float(depth_diff),
                                   C.c_float(invalid_fill), _p(dst)),
           "PyrDownDepthCPU")
    return dst


def create_vertex_map(src, K, invalid_fill):
    src = _f32(src)
    rows, cols = src.shape[:2]
    dst = np.empty((rows, cols, 3), np.float32)
    _check(lib().ref_create_vertex_map(_p(src), C.c_int64(rows),
                                       C.c_int64(cols), _p(_f64(K)),
                                       C.c_float(invalid_fill), _p(dst)),
           "CreateVertexMapCPU")
    return dst


def create_normal_map(src, invalid_fill):
    src = _f32(src)
    rows, cols = src.shape[:2]
    dst = np.empty((rows, cols, 3), np.float32)
    _check(lib().ref_create_normal_map(_p(src), C.c_int64(rows),
                                       C.c_int64(cols),
                                       C.c_float(invalid_fill), _p(dst)),
           "CreateNormalMapCPU")
    return dst


def image_to_float(src, scale, offset=0.0):
    src = np.ascontiguousarray(src)
    code = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1,
            np.dtype(np.float32): 2}[src.dtype]
    dst = np.empty(src.shape, np.float32)
    _check(lib().ref_image_to_float(_p(src), code, C.c_int64(src.size),
                                    C.c_double(scale), C.c_double(offset),
                                    _p(dst)), "ToCPU")
    return dst


def _opt32(a):
    return None if a is None else _f32(a)


def odometry(method, K, T, source_vertex, target_vertex=None,
             target_normal=None, source_depth=None, target_depth=None,
             source_intensity=None, target_intensity=None,
             target_depth_dx=None, target_depth_dy=None,
             target_intensity_dx=None, target_intensity_dy=None,
             depth_outlier_trunc=0.07, depth_huber_delta=0.05,
             intensity_huber_delta=0.1):
    """Returns (delta pose {6}, residual float, count int, A_1x29 float sums)."""
    sv = _f32(source_vertex)
    rows, cols = sv.shape[:2]
    arrs = [_opt32(a) for a in (source_depth, target_depth, source_intensity,
                                target_intensity, target_depth_dx,
                                target_depth_dy, target_intensity_dx,
                                target_intensity_dy)]
    tv, tn = _opt32(target_vertex), _opt32(target_normal)
    delta = np.zeros(6, np.float64)
    sums = np.zeros(29, np.float64)
    res, cnt = C.c_float(0), C.c_int(0)
    _check(lib().ref_odometry(int(method), rows, cols,
                              *[_p(a) for a in arrs], _p(sv), _p(tv), _p(tn),
                              _p(_f64(K)), _p(_f64(T)),
                              C.c_float(depth_outlier_trunc),
                              C.c_float(depth_huber_delta),
                              C.c_float(intensity_huber_delta), _p(delta),
                              C.byref(res), C.byref(cnt), _p(sums)),
           "ComputeOdometryResultCPU")
    return delta, res.value, cnt.value, sums


def odometry_information(source_vertex, target_vertex, K, T, square_dist_thr):
    sv, tv = _f32(source_vertex), _f32(target_vertex)
    rows, cols = sv.shape[:2]
    out = np.zeros((6, 6), np.float64)
    _check(lib().ref_odometry_information(rows, cols, _p(sv), _p(tv),
                                          _p(_f64(K)), _p(_f64(T)),
                                          C.c_float(square_dist_thr), _p(out)),
           "ComputeOdometryInformationMatrixCPU")
    return out


def extract_point_cloud(indices, nb_indices, nb_masks, block_keys, tsdf,
                        weight, color_buf, resolution, voxel_size,
                        weight_threshold, estimated_number=-1,
                        out_capacity=None):
    """The reference's ExtractPointCloudCPU body: (points, normals,
    colors|None, total_count). Output order is sequential only under
    set_threads(1)."""
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    nb_indices = np.ascontiguousarray(nb_indices, dtype=np.int32)
    nb_masks = np.ascontiguousarray(nb_masks, dtype=np.uint8)
    block_keys = np.ascontiguousarray(block_keys, dtype=np.int32)
    n = indices.shape[0]
    capacity = block_keys.shape[0]
    grid_is_f32 = int(weight.dtype == np.float32)
    cap = int(out_capacity if out_capacity is not None else
              (estimated_number if estimated_number >= 0
               else n * resolution ** 3 * 3))
    pts = np.zeros((cap, 3), np.float32)
    nrm = np.zeros((cap, 3), np.float32)
    col = np.zeros((cap, 3), np.float32) if color_buf is not None else None
    L = lib()
    L.ref_extract_point_cloud.restype = C.c_int64
    total = int(L.ref_extract_point_cloud(
        _p(indices), _p(nb_indices), _p(nb_masks), _p(block_keys),
        C.c_int64(capacity), _p(tsdf), _p(weight), _p(color_buf), grid_is_f32,
        C.c_int64(n), int(resolution), C.c_float(voxel_size),
        C.c_float(weight_threshold), _p(pts), _p(nrm), _p(col),
        C.c_int64(cap), int(estimated_number)))
    if total < 0:
        raise RuntimeError("extract_point_cloud: %s"
                           % L.ref_last_error().decode())
    m = min(total, cap)
    return pts[:m], nrm[:m], (None if col is None else col[:m]), total


def estimate_covariances(points, indices, counts):
    points = np.ascontiguousarray(points)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    n, max_nn = indices.shape
    cov = np.zeros((n, 3, 3), points.dtype)
    _check(lib().ref_estimate_covariances(
        _p(points), _p(indices), _p(counts), C.c_int64(n), int(max_nn),
        int(points.dtype == np.float64), _p(cov)), "estimate_covariances")
    return cov


def svd3x3(A):
    A = np.ascontiguousarray(A)
    U, S, V = np.zeros((3, 3), A.dtype), np.zeros(3, A.dtype), \
        np.zeros((3, 3), A.dtype)
    _check(lib().ref_svd3x3(_p(A), int(A.dtype == np.float64), _p(U), _p(S),
                            _p(V)), "svd3x3")
    return U, S, V


def solve_svd3x3(A, b):
    A = np.ascontiguousarray(A)
    b = np.ascontiguousarray(b, dtype=A.dtype)
    x = np.zeros(3, A.dtype)
    _check(lib().ref_solve_svd3x3(_p(A), _p(b), int(A.dtype == np.float64),
                                  _p(x)), "solve_svd3x3")
    return x


def estimate_color_gradients(points, normals, colors, indices, counts):
    points = np.ascontiguousarray(points)
    dt = points.dtype
    normals = np.ascontiguousarray(normals, dtype=dt)
    colors = np.ascontiguousarray(colors, dtype=dt)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    n, max_nn = indices.shape
    g = np.zeros((n, 3), dt)
    _check(lib().ref_estimate_color_gradients(
        _p(points), _p(normals), _p(colors), _p(indices), _p(counts),
        C.c_int64(n), int(max_nn), int(dt == np.float64), _p(g)),
        "estimate_color_gradients")
    return g


def normals_from_covariances(cov, normals=None):
    cov = np.ascontiguousarray(cov)
    n = cov.shape[0]
    has = normals is not None
    out = np.ascontiguousarray(normals, dtype=cov.dtype).copy() if has \
        else np.zeros((n, 3), cov.dtype)
    _check(lib().ref_normals_from_covariances(
        _p(cov), C.c_int64(n), int(cov.dtype == np.float64), _p(out),
        int(has)), "normals_from_covariances")
    return out


def extract_triangle_mesh(indices, nb_indices, nb_masks, block_keys, tsdf,
                          weight, color_buf, resolution, voxel_size,
                          weight_threshold):
    """The reference's ExtractTriangleMeshCPU body, counting pass included:
    (vertices, normals, colors|None, triangles). inv_block_indices is built
    here as VoxelBlockGrid::ExtractTriangleMesh builds it. Output order is
    sequential only under set_threads(1)."""
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    nb_indices = np.ascontiguousarray(nb_indices, dtype=np.int32)
    nb_masks = np.ascontiguousarray(nb_masks, dtype=np.uint8)
    block_keys = np.ascontiguousarray(block_keys, dtype=np.int32)
    n = indices.shape[0]
    capacity = block_keys.shape[0]
    inv = np.full(capacity, -1, np.int32)
    inv[indices] = np.arange(n, dtype=np.int32)
    grid_is_f32 = int(weight.dtype == np.float32)
    vcap = n * resolution ** 3 * 3
    tcap = 3 * vcap
    pts = np.zeros((vcap, 3), np.float32)
    nrm = np.zeros((vcap, 3), np.float32)
    col = np.zeros((vcap, 3), np.float32) if color_buf is not None else None
    tri = np.zeros((tcap, 3), np.int32)
    nv, nt = C.c_int64(0), C.c_int64(0)
    _check(lib().ref_extract_triangle_mesh(
        _p(indices), _p(inv), _p(nb_indices), _p(nb_masks), _p(block_keys),
        C.c_int64(capacity), _p(tsdf), _p(weight), _p(color_buf), grid_is_f32,
        C.c_int64(n), int(resolution), C.c_float(voxel_size),
        C.c_float(weight_threshold), _p(pts), _p(nrm), _p(col),
        C.c_int64(vcap), _p(tri), C.c_int64(tcap), C.byref(nv), C.byref(nt)),
        "ref_extract_triangle_mesh")
    m, k = nv.value, nt.value
    assert m <= vcap and k <= tcap
    return pts[:m], nrm[:m], (None if col is None else col[:m]), tri[:k]


# ---- FPFH (FeatureCPU.cpp + FeatureImpl.h) ---------------------------------

def fpfh_float_math_is_float():
    """Whether unqualified acos(float) is the float overload where the
    reference's ComputePairFeature was compiled (it is the C function of
    double when FeatureCPU.cpp is a translation unit of its own)."""
    return bool(lib().ref_fpfh_float_math_is_float())


def fpfh_pair_feature(p1, n1, p2, n2, dtype=np.float64):
    """ComputePairFeature on one pair -> (f0, f1, f2, f3) of `dtype`."""
    a = [np.ascontiguousarray(v, dtype=dtype) for v in (p1, n1, p2, n2)]
    out = np.zeros(4, dtype)
    _check(lib().ref_fpfh_pair_feature(
        *[_p(v) for v in a], int(np.dtype(dtype) == np.float64), _p(out)),
        "ComputePairFeature")
    return tuple(out)


def fpfh_from_lists(points, normals, idx, d2, counts=None, splits=None,
                    list_points=None, mask=None, into=None):
    """ComputeFPFHFeatureCPU, the arguments of _fpfh_oracle.fpfh_from_lists:
    padded lists (idx / d2 {R, W} with counts) or CSR lists (idx / d2 1-d with
    splits). The filtered form takes list_points (the body's
    map_info_idx_to_point_idx) and mask (bool {n}); the output then has one
    row per masked point. The body adds into `into` (default zeros)."""
    points = np.ascontiguousarray(points)
    dt = points.dtype
    normals = np.ascontiguousarray(normals, dtype=dt)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    d2 = np.ascontiguousarray(d2, dtype=dt)
    n = points.shape[0]
    if splits is not None:
        splits = np.ascontiguousarray(splits, dtype=np.int64)
        rows, width, counts = splits.shape[0] - 1, 0, None
        assert idx.ndim == 1 and idx.shape[0] == d2.shape[0] == splits[-1]
    else:
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        rows, width = idx.shape
        assert d2.shape == idx.shape and counts.shape == (rows,)
    assert (mask is None) == (list_points is None)
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        list_points = np.ascontiguousarray(list_points, dtype=np.int64)
        n_out = int(mask.sum())
    else:
        n_out = n
    out = (np.zeros((n_out, 33), dt) if into is None
           else np.ascontiguousarray(into, dtype=dt).copy())
    assert out.shape == (n_out, 33)
    _check(lib().ref_fpfh_from_neighbors(
        _p(points), _p(normals), C.c_int64(n), int(dt == np.float64), _p(idx),
        _p(d2), _p(counts), _p(splits), int(width), C.c_int64(rows), _p(mask),
        _p(list_points), _p(out), C.c_int64(n_out)), "ComputeFPFHFeatureCPU")
    return out


# ---- Doppler ICP (RegistrationCPU.cpp:335-493) -------------------------------

def doppler_precompute(R, r, w, v):
    """PreComputeForDopplerICPKernelCPU -> v_s_in_S {3} of the inputs' dtype."""
    dt = np.asarray(R).dtype
    a = [np.ascontiguousarray(x, dtype=dt) for x in (R, r, w, v)]
    out = np.zeros(3, dt)
    _check(lib().ref_doppler_precompute(*[_p(x) for x in a],
                                        int(dt == np.float64), _p(out)),
           "PreComputeForDopplerICPKernelCPU")
    return out


def doppler_dual_dispatch_accepts(method_geometric, method_doppler):
    """Whether DISPATCH_DUAL_ROBUST_KERNEL_FUNCTION takes this pair."""
    return bool(lib().ref_doppler_dual_dispatch_accepts(int(method_geometric),
                                                        int(method_doppler)))


def doppler_pair_terms(src, dopplers, directions, tgt, tgt_n, corr, R, r, w, v,
                       period, reject, threshold, kernel_geometric,
                       kernel_doppler, lambda_doppler, dual=None):
    """The arguments of _doppler_oracle.pair_terms -> terms {n, 29} of the
    point dtype, one row per SOURCE row (a row without a correspondence is
    29 zeros). dual: weights from the reference's dual dispatch (default where
    it accepts the pair) or from its single-kernel dispatch per term."""
    src = np.ascontiguousarray(src)
    dt = src.dtype
    dopplers, directions, tgt, tgt_n = (
        np.ascontiguousarray(a, dtype=dt)
        for a in (dopplers, directions, tgt, tgt_n))
    corr = np.ascontiguousarray(corr, dtype=np.int64).reshape(-1)
    R, r = (np.ascontiguousarray(a, dtype=dt) for a in (R, r))
    vs = doppler_precompute(R, r, np.asarray(w, dt), np.asarray(v, dt))
    if dual is None:
        dual = doppler_dual_dispatch_accepts(kernel_geometric[0],
                                             kernel_doppler[0])
    n = src.shape[0]
    out = np.zeros((n, 29), dt)
    _check(lib().ref_doppler_pair_terms(
        _p(src), _p(dopplers), _p(directions), _p(tgt), _p(tgt_n), _p(corr),
        C.c_int64(n), int(dt == np.float64), _p(R), _p(r), _p(vs),
        int(bool(reject)), C.c_double(threshold), C.c_double(lambda_doppler),
        C.c_double(period), int(kernel_geometric[0]),
        C.c_double(kernel_geometric[1]), C.c_double(kernel_geometric[2]),
        int(kernel_doppler[0]), C.c_double(kernel_doppler[1]),
        C.c_double(kernel_doppler[2]), int(bool(dual)), _p(out)),
        "ComputePoseDopplerICPKernelCPU")
    return out


# ---- SLAC fill-ins (FillInLinearSystemCPU.cpp + FillInLinearSystemImpl.h) ----

def fill_in_rigid_alignment_term(AtA, Atb, residual, p, q, n, i, j, threshold):
    """FillInRigidAlignmentTermCPU on copies of float32 AtA {V,V}, Atb {V},
    residual {1} -> (AtA, Atb, residual)."""
    AtA, Atb, residual = (np.ascontiguousarray(a, dtype=np.float32).copy()
                          for a in (AtA, Atb, residual))
    p, q, n = _f32(p), _f32(q), _f32(n)
    _check(lib().ref_fill_in_rigid_alignment_term(
        _p(AtA), _p(Atb), _p(residual), C.c_int64(Atb.shape[0]), _p(p), _p(q),
        _p(n), C.c_int64(p.shape[0]), int(i), int(j), C.c_float(threshold)),
        "FillInRigidAlignmentTermCPU")
    return AtA, Atb, residual


def fill_in_rigid_alignment_pairs(p, q, n, threshold):
    """One call per pair, (i, j) = (0, 1), into zeros -> (A {m,12,12},
    b {m,12}, r2 {m}) float32."""
    p, q, n = _f32(p), _f32(q), _f32(n)
    m = p.shape[0]
    out = np.zeros((m, 157), np.float32)
    _check(lib().ref_fill_in_rigid_alignment_pairs(
        _p(p), _p(q), _p(n), C.c_int64(m), C.c_float(threshold), _p(out)),
        "FillInRigidAlignmentTermCPU per pair")
    return (out[:, :144].reshape(m, 12, 12).copy(), out[:, 144:156].copy(),
            out[:, 156].copy())


def _seam(arrays):
    p, q, cn, n, v, ip, iq, rp, rq = arrays
    f = [_f32(a) for a in (p, q, cn, n, v)]
    ix = [np.ascontiguousarray(a, dtype=np.int32) for a in (ip, iq)]
    rt = [_f32(a) for a in (rp, rq)]
    return f + ix + rt


def fill_in_slac_alignment_term(AtA, Atb, residual, arrays, i, j, n_frags,
                                threshold):
    """FillInSLACAlignmentTermCPU on copies; arrays as
    _slac_nonrigid_oracle.pair_jacobians takes them (..., idx_ps, idx_qs,
    ratio_ps, ratio_qs)."""
    AtA, Atb, residual = (np.ascontiguousarray(a, dtype=np.float32).copy()
                          for a in (AtA, Atb, residual))
    a = _seam(arrays)
    _check(lib().ref_fill_in_slac_alignment_term(
        _p(AtA), _p(Atb), _p(residual), C.c_int64(Atb.shape[0]),
        *[_p(x) for x in a], C.c_int64(a[0].shape[0]), int(i), int(j),
        int(n_frags), C.c_float(threshold)), "FillInSLACAlignmentTermCPU")
    return AtA, Atb, residual


def fill_in_slac_alignment_pairs(arrays, i, j, n_frags, threshold, n_vars):
    """One call per pair into a zeroed system of n_vars unknowns -> (A
    {m,V,V}, b {m,V}, r2 {m}) float32."""
    a = _seam(arrays)
    m = a[0].shape[0]
    stride = n_vars * n_vars + n_vars + 1
    out = np.zeros((m, stride), np.float32)
    _check(lib().ref_fill_in_slac_alignment_pairs(
        C.c_int64(n_vars), *[_p(x) for x in a], C.c_int64(m), int(i), int(j),
        int(n_frags), C.c_float(threshold), _p(out)),
        "FillInSLACAlignmentTermCPU per pair")
    V = n_vars
    return (out[:, :V * V].reshape(m, V, V), out[:, V * V:V * V + V],
            out[:, -1])


def fill_in_slac_regularizer_term(grid_idx, nbs_idx, nbs_mask, init, curr,
                                  weight, n_frags, anchor_idx, n):
    """FillInSLACRegularizerTermCPU into zeros, the arguments of
    _slac_nonrigid_oracle.regularizer -> dict(AtA, Atb, residual) float32."""
    grid_idx = np.ascontiguousarray(grid_idx, dtype=np.int32)
    nbs_idx = np.ascontiguousarray(nbs_idx, dtype=np.int32)
    nbs_mask = np.ascontiguousarray(np.asarray(nbs_mask) != 0, dtype=np.uint8)
    init, curr = _f32(init), _f32(curr)
    AtA = np.zeros((n, n), np.float32)
    Atb = np.zeros(n, np.float32)
    res = np.zeros(1, np.float32)
    _check(lib().ref_fill_in_slac_regularizer_term(
        _p(AtA), _p(Atb), _p(res), C.c_int64(n), _p(grid_idx), _p(nbs_idx),
        _p(nbs_mask), _p(init), _p(curr), C.c_int64(grid_idx.shape[0]),
        C.c_int64(init.shape[0]), C.c_float(weight), int(n_frags),
        int(anchor_idx)), "FillInSLACRegularizerTermCPU")
    return dict(AtA=AtA, Atb=Atb, residual=float(res[0]))
