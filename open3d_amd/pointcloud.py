"""Mirror of t::geometry::PointCloud's selection, filter, sampling, cropping,
smoothing, boundary, normal-orientation, segmentation, metrics, convex-hull,
hidden-point-removal and oriented bounding box / ellipsoid methods
(t/geometry/PointCloud.cpp:435-494, 569-854, 986-1050, 1074-1203, 1634-1720,
1805-1836) on the HIP backend.

A cloud is a dict of CUDA attribute tensors with "positions" ({N,3} Float32 or
Float64) required; every other attribute has N rows of any width and dtype
("normals", uint8 "colors", ...). Each function returns (attrs_out, mask) as
the reference's (PointCloud, Tensor) tuples do; mask is a bool {N} tensor.
"""
import ctypes as C

import torch

from . import _lib
from .core import TORCH_TO_O3DMI, require_cuda, stream

MAX_ATTRS = 8  # attributes moved by one compaction launch


def _positions(attrs):
    if "positions" not in attrs:
        raise ValueError('a cloud needs "positions"')
    p = require_cuda(attrs["positions"], "positions")
    if p.dim() != 2 or p.shape[1] != 3 or p.dtype not in (torch.float32,
                                                          torch.float64):
        raise ValueError("positions must be {N,3} Float32 or Float64")
    return p.contiguous()


def _rows(attrs):
    p = _positions(attrs)
    n = p.shape[0]
    out = {}
    for name, t in attrs.items():
        t = p if name == "positions" else require_cuda(t, name).contiguous()
        if t.dim() < 1 or t.shape[0] != n:
            raise ValueError("attribute %r must have %d rows" % (name, n))
        out[name] = t
    return out, n


def _row_bytes(t):
    w = t.element_size()
    for d in t.shape[1:]:
        w *= d
    return w


def _tables(ins, outs):
    k = len(ins)
    return ((C.c_void_p * k)(*[t.data_ptr() for t in ins]),
            (C.c_int64 * k)(*[_row_bytes(t) for t in ins]),
            (C.c_void_p * k)(*[t.data_ptr() for t in outs]))


def _select(attrs, rows_out, call, where):
    """Runs `call(n_attrs, in, row_bytes, out, m)` over the attributes in
    groups of MAX_ATTRS and trims the outputs to the rows kept."""
    attrs, _ = _rows(attrs)
    names = list(attrs)
    out = {}
    for g in range(0, len(names), MAX_ATTRS):
        group = names[g:g + MAX_ATTRS]
        ins = [attrs[k] for k in group]
        outs = [torch.empty((rows_out,) + tuple(t.shape[1:]), dtype=t.dtype,
                            device=t.device) for t in ins]
        m = C.c_int64(0)
        a_in, widths, a_out = _tables(ins, outs)
        _lib.check(call(len(group), a_in, widths, a_out, C.byref(m)), where)
        for k, t in zip(group, outs):
            out[k] = t[:m.value]
    return out


def _mask_u8(mask, n):
    mask = require_cuda(mask, "mask")
    if mask.dtype not in (torch.bool, torch.uint8) or mask.shape != (n,):
        raise ValueError("mask must be a bool {N} tensor")
    return mask.contiguous().view(torch.uint8)


def select_by_mask(attrs, mask, invert=False):
    """PointCloud::SelectByMask: the rows with mask != invert, in input
    order. -> (attrs_out, mask)."""
    _, n = _rows(attrs)
    m8 = _mask_u8(mask, n)
    out = _select(
        attrs, n,
        lambda k, a, w, o, m: _lib.lib().o3dmi_pointcloud_select_by_mask(
            n, _lib.ptr(m8), int(bool(invert)), k, a, w, o, m, stream()),
        "select_by_mask")
    return out, m8.view(torch.bool)


def select_by_index(attrs, indices, invert=False, remove_duplicates=False):
    """PointCloud::SelectByIndex: a row gather (duplicates repeat), or, with
    invert / remove_duplicates, index -> mask -> select_by_mask.
    -> (attrs_out, indices)."""
    _, n = _rows(attrs)
    indices = require_cuda(indices, "indices")
    if indices.dtype != torch.int64 or indices.dim() != 1:
        raise ValueError("indices must be an Int64 {M} tensor")
    indices = indices.contiguous()
    cnt = indices.shape[0]
    by_mask = bool(invert) or bool(remove_duplicates)
    out = _select(
        attrs, n if by_mask else cnt,
        lambda k, a, w, o, m: _lib.lib().o3dmi_pointcloud_select_by_index(
            n, _lib.ptr(indices), cnt, int(bool(invert)),
            int(bool(remove_duplicates)), k, a, w, o, m, stream()),
        "select_by_index")
    return out, indices


def _filtered(attrs, mask8):
    out, _ = select_by_mask(attrs, mask8)
    return out, mask8.view(torch.bool)


def remove_non_finite_points(attrs, remove_nan=True, remove_inf=True):
    """PointCloud::RemoveNonFinitePoints -> (attrs_out, mask)."""
    p = _positions(attrs)
    n = p.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=p.device)
    m = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_pointcloud_remove_non_finite_points(
        _lib.ptr(p), n, TORCH_TO_O3DMI[p.dtype], int(bool(remove_nan)),
        int(bool(remove_inf)), _lib.ptr(mask), C.byref(m), stream()),
        "remove_non_finite_points")
    return _filtered(attrs, mask)


def remove_duplicated_points(attrs):
    """PointCloud::RemoveDuplicatedPoints: points are equal when their bits
    are; the lowest index of each survives. -> (attrs_out, mask)."""
    p = _positions(attrs)
    n = p.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=p.device)
    m = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_pointcloud_remove_duplicated_points(
        _lib.ptr(p), n, TORCH_TO_O3DMI[p.dtype], _lib.ptr(mask), C.byref(m),
        stream()), "remove_duplicated_points")
    return _filtered(attrs, mask)


def remove_radius_outliers(attrs, nb_points, search_radius):
    """PointCloud::RemoveRadiusOutliers: keeps the points with at least
    nb_points points (themselves included) within search_radius.
    -> (attrs_out, mask)."""
    p = _positions(attrs)
    n = p.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=p.device)
    m = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_pointcloud_remove_radius_outliers(
        _lib.ptr(p), n, TORCH_TO_O3DMI[p.dtype], int(nb_points),
        C.c_double(search_radius), _lib.ptr(mask), C.byref(m), stream()),
        "remove_radius_outliers")
    return _filtered(attrs, mask)


def statistical_outlier_mask(positions, nb_neighbors, std_ratio):
    """The filter alone: -> (mask uint8 {N}, avg_distances {N}, dict(mean,
    std, threshold, kept))."""
    p = _positions({"positions": positions})
    n = p.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=p.device)
    avg = torch.empty(n, dtype=p.dtype, device=p.device)
    stats = (C.c_double * 3)(float("nan"), float("nan"), float("nan"))
    m = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_pointcloud_remove_statistical_outliers(
        _lib.ptr(p), n, TORCH_TO_O3DMI[p.dtype], int(nb_neighbors),
        C.c_double(std_ratio), _lib.ptr(mask), _lib.ptr(avg), stats,
        C.byref(m), stream()), "remove_statistical_outliers")
    return mask, avg, dict(mean=stats[0], std=stats[1], threshold=stats[2],
                           kept=m.value)


def remove_statistical_outliers(attrs, nb_neighbors, std_ratio,
                                return_stats=False):
    """PointCloud::RemoveStatisticalOutliers -> (attrs_out, mask), and with
    return_stats a dict(mean, std, threshold, kept, avg_distances) as well."""
    mask, avg, stats = statistical_outlier_mask(_positions(attrs),
                                                nb_neighbors, std_ratio)
    out, mask = _filtered(attrs, mask)
    if return_stats:
        stats["avg_distances"] = avg
        return out, mask, stats
    return out, mask


# ---- sampling, cropping, bounds -----------------------------------------------

def uniform_down_sample(attrs, every_k_points):
    """PointCloud::UniformDownSample: rows 0, k, 2 k, ... of every attribute."""
    _, n = _rows(attrs)
    k = int(every_k_points)
    if k < 1:
        raise ValueError(
            "Illegal sample rate, every_k_points must be larger than 0.")
    return _select(
        attrs, (n + k - 1) // k,
        lambda c, a, w, o, m: _lib.lib().o3dmi_pointcloud_uniform_down_sample(
            n, k, c, a, w, o, m, stream()),
        "uniform_down_sample")


def random_sample_indices(n, sampling_ratio, seed=0, device="cuda"):
    """The Int64 {int(ratio * n)} indices random_down_sample gathers: entries
    0 .. m-1 of the permutation of [0, n) that seed selects."""
    indices = torch.empty(n, dtype=torch.int64, device=device)
    m = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_pointcloud_random_sample_indices(
        n, C.c_double(sampling_ratio),
        C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _lib.ptr(indices),
        C.byref(m), stream()), "random_down_sample")
    return indices[:m.value]


def random_down_sample(attrs, sampling_ratio, seed=0):
    """PointCloud::RandomDownSample: int(ratio * N) distinct rows in shuffled
    order. The sample is a pure function of (seed, N), the same on every run
    (upstream draws from its global engine)."""
    p = _positions(attrs)
    indices = random_sample_indices(p.shape[0], sampling_ratio, seed, p.device)
    out, _ = select_by_index(attrs, indices)
    return out


def farthest_point_order(positions, num_samples, start_index=0, form=0):
    """The Int64 {num_samples} order in which FarthestPointDownSample picks
    its samples. form: 0 by size, 1 resident, 2 streamed (same bits)."""
    p = _positions({"positions": positions})
    order = torch.empty(int(num_samples), dtype=torch.int64, device=p.device)
    _lib.check(_lib.lib().o3dmi_pointcloud_farthest_point_order(
        _lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype], int(num_samples),
        int(start_index), int(form), _lib.ptr(order), stream()),
        "farthest_point_order")
    return order


def farthest_point_mask(positions, num_samples, start_index=0,
                        return_order=False):
    """The filter alone: -> (mask uint8 {N}, kept) and, with return_order,
    the Int64 {num_samples} order as well."""
    p = _positions({"positions": positions})
    n = p.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=p.device)
    order = torch.empty(int(num_samples), dtype=torch.int64,
                        device=p.device) if return_order else None
    m = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_pointcloud_farthest_point_down_sample(
        _lib.ptr(p), n, TORCH_TO_O3DMI[p.dtype], int(num_samples),
        int(start_index), _lib.ptr(mask),
        _lib.ptr(order) if order is not None else None, C.byref(m), stream()),
        "farthest_point_down_sample")
    if return_order:
        return mask, m.value, order
    return mask, m.value


def farthest_point_down_sample(attrs, num_samples, start_index=0,
                               return_order=False):
    """PointCloud::FarthestPointDownSample: the chosen rows in input order.
    Ties go to the lowest index; a cloud with fewer than num_samples distinct
    points gives fewer rows. With return_order -> (attrs_out, order)."""
    res = farthest_point_mask(_positions(attrs), num_samples, start_index,
                              return_order)
    out, _ = _filtered(attrs, res[0])
    if return_order:
        return out, res[2]
    return out


def _mask_call(attrs, call, where):
    p = _positions(attrs)
    n = p.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=p.device)
    m = C.c_int64(0)
    _lib.check(call(_lib.ptr(p), n, TORCH_TO_O3DMI[p.dtype], _lib.ptr(mask),
                    C.byref(m), stream()), where)
    return mask


def _cropped(attrs, mask, invert):
    out, _ = select_by_mask(attrs, mask, invert)
    return out


def crop(attrs, min_bound=None, max_bound=None, center=None, rotation=None,
         extent=None, invert=False):
    """PointCloud::Crop with an axis-aligned box (min_bound, max_bound) or an
    oriented one (center, rotation {3,3}, extent): the rows inside, both ends
    inclusive, or with invert the rows outside. An empty box (zero volume)
    gives an empty cloud, or a copy under invert, as upstream."""
    aabb = min_bound is not None and max_bound is not None
    obb = center is not None and rotation is not None and extent is not None
    if aabb == obb or (aabb or obb) != any(
            v is not None
            for v in (min_bound, max_bound, center, rotation, extent)):
        raise ValueError("crop needs (min_bound, max_bound) or "
                         "(center, rotation, extent)")
    if aabb:
        lo, hi = _vec3(min_bound, "min_bound"), _vec3(max_bound, "max_bound")
        size = [hi[k] - lo[k] for k in range(3)]

        def call(p, n, dtype, mask, m, st):
            return _lib.lib().o3dmi_pointcloud_aabb_mask(p, n, dtype, lo, hi,
                                                         mask, m, st)
    else:
        c, size = _vec3(center, "center"), _vec3(extent, "extent")
        r = [float(x) for row in (rotation.tolist() if hasattr(
            rotation, "tolist") else rotation) for x in row]
        if len(r) != 9:
            raise ValueError("rotation must have shape {3,3}")
        rot = (C.c_double * 9)(*r)

        def call(p, n, dtype, mask, m, st):
            return _lib.lib().o3dmi_pointcloud_obb_mask(p, n, dtype, c, rot,
                                                        size, mask, m, st)
    if min(size) < 0:
        raise ValueError("the box has a negative extent")
    if size[0] * size[1] * size[2] == 0:  # upstream's IsEmpty()
        _, n = _rows(attrs)
        p = _positions(attrs)
        mask = torch.zeros(n, dtype=torch.uint8, device=p.device)
        return _cropped(attrs, mask, invert)
    return _cropped(attrs, _mask_call(attrs, call, "crop"), invert)


def get_min_max_bound(attrs):
    """(GetMinBound, GetMaxBound) as Float64 {3} host tensors; zeros for an
    empty cloud, as upstream."""
    p = _positions(attrs)
    lo, hi = (C.c_double * 3)(), (C.c_double * 3)()
    _lib.check(_lib.lib().o3dmi_pointcloud_min_max_bound(
        _lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype], lo, hi, stream()),
        "get_min_max_bound")
    return (torch.tensor(list(lo), dtype=torch.float64),
            torch.tensor(list(hi), dtype=torch.float64))


def get_min_bound(attrs):
    """PointCloud::GetMinBound."""
    return get_min_max_bound(attrs)[0]


def get_max_bound(attrs):
    """PointCloud::GetMaxBound."""
    return get_min_max_bound(attrs)[1]


# ---- metrics and nearest-point distances ---------------------------------------

class Metric:
    """t::geometry::Metric, in upstream's enum order."""
    ChamferDistance = 0
    HausdorffDistance = 1
    FScore = 2


def compute_point_cloud_distance(attrs, target_attrs, return_index=False):
    """PointCloud::ComputePointCloudDistance: for every point of the cloud the
    distance to the nearest point of the target, {N} in the point dtype; with
    return_index also the Int32 {N} index of that point (ties: the lowest)."""
    p, t = _positions(attrs), _positions(target_attrs)
    if p.dtype != t.dtype:
        raise ValueError("both clouds must have the same dtype")
    q = p.shape[0]
    dist = torch.empty(q, dtype=p.dtype, device=p.device)
    idx = torch.empty(q, dtype=torch.int32,
                      device=p.device) if return_index else None
    _lib.check(_lib.lib().o3dmi_pointcloud_nearest_distance(
        _lib.ptr(t), t.shape[0], _lib.ptr(p), q, TORCH_TO_O3DMI[p.dtype],
        _lib.ptr(dist), _lib.ptr(idx), stream()),
        "compute_point_cloud_distance")
    if return_index:
        return dist, idx
    return dist


def compute_metrics(attrs1, attrs2, metrics, fscore_radius=(0.01,),
                    return_raw=False):
    """PointCloud::ComputeMetrics -> a CPU Float32 tensor with the values in the
    order of `metrics` (Metric codes); every FScore entry expands to one value
    per radius. With return_raw also a dict(sum, max, counts,
    second_pass_queries), each with the direction 1 -> 2 first."""
    p1, p2 = _positions(attrs1), _positions(attrs2)
    if p1.dtype != p2.dtype:
        raise ValueError("both clouds must have the same dtype")
    codes = [int(m) for m in metrics]
    radii = [float(r) for r in fscore_radius]
    n_values = sum(len(radii) if m == Metric.FScore else 1 for m in codes)
    values = (C.c_float * max(n_values, 1))()
    counts = (C.c_int64 * max(2 * len(radii), 1))()
    raw = _lib.MetricsRawC()
    raw.counts = C.cast(counts, C.POINTER(C.c_int64))
    _lib.check(_lib.lib().o3dmi_pointcloud_compute_metrics(
        _lib.ptr(p1), p1.shape[0], _lib.ptr(p2), p2.shape[0],
        TORCH_TO_O3DMI[p1.dtype], (C.c_int * max(len(codes), 1))(*codes),
        len(codes), (C.c_float * max(len(radii), 1))(*radii), len(radii),
        values, n_values, C.byref(raw), stream()), "compute_metrics")
    out = torch.tensor(list(values)[:n_values], dtype=torch.float32)
    if not return_raw:
        return out
    r = len(radii)
    return out, dict(sum=list(raw.sum), max=list(raw.max),
                     counts=[list(counts)[:r], list(counts)[r:2 * r]],
                     second_pass_queries=list(raw.second_pass_queries))


# ---- smoothing, boundary detection, normal orientation ------------------------
# Each returns a new cloud dict: "positions" (and "normals" where the operator
# moves them) replaced, every other attribute carried through unchanged.

def _normals(attrs, p, required):
    if "normals" not in attrs:
        if required:
            raise ValueError(required)
        return None
    nrm = require_cuda(attrs["normals"], "normals")
    if nrm.shape != p.shape or nrm.dtype != p.dtype:
        raise ValueError("normals must match positions in shape and dtype")
    return nrm.contiguous()


def _carried(attrs, **replaced):
    out = dict(attrs)
    out.update(replaced)
    return out


def smooth_laplacian(attrs, iterations=10, lambda_=0.5, max_nn=20,
                     use_fixed_neighborhoods=False):
    """PointCloud::SmoothLaplacian. max_nn defaults to 20, as in upstream's
    header (t/geometry/PointCloud.h:590), not to the 30 of the other
    operators."""
    p = _positions(attrs)
    out = torch.empty_like(p)
    _lib.check(_lib.lib().o3dmi_pointcloud_smooth_laplacian(
        _lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype], int(iterations),
        C.c_double(lambda_), int(max_nn), int(bool(use_fixed_neighborhoods)),
        _lib.ptr(out), stream()), "smooth_laplacian")
    return _carried(attrs, positions=out)


def smooth_taubin(attrs, iterations=10, lambda_=0.5, mu=-0.53, max_nn=20,
                  use_fixed_neighborhoods=False):
    """PointCloud::SmoothTaubin. max_nn defaults to 20, as in upstream's
    header (t/geometry/PointCloud.h:610)."""
    p = _positions(attrs)
    out = torch.empty_like(p)
    _lib.check(_lib.lib().o3dmi_pointcloud_smooth_taubin(
        _lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype], int(iterations),
        C.c_double(lambda_), C.c_double(mu), int(max_nn),
        int(bool(use_fixed_neighborhoods)), _lib.ptr(out), stream()),
        "smooth_taubin")
    return _carried(attrs, positions=out)


def smooth_mls(attrs, radius=0.05, max_nn=30):
    """PointCloud::SmoothMLS; a cloud with normals gets the plane normals."""
    p = _positions(attrs)
    nrm = _normals(attrs, p, None)
    out = torch.empty_like(p)
    out_n = torch.empty_like(nrm) if nrm is not None else None
    _lib.check(_lib.lib().o3dmi_pointcloud_smooth_mls(
        _lib.ptr(p), _lib.ptr(nrm) if nrm is not None else None, p.shape[0],
        TORCH_TO_O3DMI[p.dtype], C.c_double(radius), int(max_nn),
        _lib.ptr(out), _lib.ptr(out_n) if out_n is not None else None,
        stream()), "smooth_mls")
    if out_n is None:
        return _carried(attrs, positions=out)
    return _carried(attrs, positions=out, normals=out_n)


def smooth_bilateral(attrs, radius=0.05, max_nn=30, sigma_s=0.05,
                     sigma_r=0.05):
    """PointCloud::SmoothBilateral; a cloud without normals gets them from
    EstimateNormals with upstream's defaults (KNN, 30) first."""
    p = _positions(attrs)
    n = p.shape[0]
    if n == 0:
        return _carried(attrs, positions=p.clone())
    if sigma_s <= 0 or sigma_r <= 0:
        raise ValueError("Sigma values must be positive.")
    nrm = _normals(attrs, p, None)
    if nrm is None:
        nrm = torch.empty_like(p)
        _lib.check(_lib.lib().o3dmi_pointcloud_estimate_normals(
            _lib.ptr(p), n, TORCH_TO_O3DMI[p.dtype], 30, C.c_double(-1.0),
            _lib.ptr(nrm), 0, stream()), "estimate_normals")
    out = torch.empty_like(p)
    _lib.check(_lib.lib().o3dmi_pointcloud_smooth_bilateral(
        _lib.ptr(p), _lib.ptr(nrm), n, TORCH_TO_O3DMI[p.dtype],
        C.c_double(radius), int(max_nn), C.c_double(sigma_s),
        C.c_double(sigma_r), _lib.ptr(out), stream()), "smooth_bilateral")
    return _carried(attrs, positions=out, normals=nrm)


def compute_boundary_points(attrs, radius, max_nn=30, angle_threshold=90.0):
    """PointCloud::ComputeBoundaryPoints -> (boundary cloud, mask)."""
    p = _positions(attrs)
    nrm = _normals(attrs, p, "PointCloud must have normals attribute to "
                   "compute boundary points.")
    n = p.shape[0]
    mask = torch.zeros(n, dtype=torch.uint8, device=p.device)
    m = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_pointcloud_compute_boundary_points(
        _lib.ptr(p), _lib.ptr(nrm), n, TORCH_TO_O3DMI[p.dtype],
        C.c_double(radius), int(max_nn), C.c_double(angle_threshold),
        _lib.ptr(mask), C.byref(m), stream()), "compute_boundary_points")
    return _filtered(attrs, mask)


def normalize_normals(attrs):
    """PointCloud::NormalizeNormals; a cloud without normals is returned as
    it is (upstream warns)."""
    p = _positions(attrs)
    nrm = _normals(attrs, p, None)
    if nrm is None:
        return dict(attrs)
    nrm = nrm.clone()
    _lib.check(_lib.lib().o3dmi_pointcloud_normalize_normals(
        _lib.ptr(nrm), p.shape[0], TORCH_TO_O3DMI[p.dtype], stream()),
        "normalize_normals")
    return _carried(attrs, normals=nrm)


def _vec3(v, name):
    v = [float(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]
    if len(v) != 3:
        raise ValueError("%s must have shape {3}" % name)
    return (C.c_double * 3)(*v)


def orient_normals_to_align_with_direction(attrs,
                                           orientation_reference=(0.0, 0.0,
                                                                  1.0)):
    """PointCloud::OrientNormalsToAlignWithDirection."""
    p = _positions(attrs)
    nrm = _normals(attrs, p, "No normals in the PointCloud. Call "
                   "EstimateNormals() first.").clone()
    _lib.check(
        _lib.lib().o3dmi_pointcloud_orient_normals_to_align_with_direction(
            _lib.ptr(nrm), p.shape[0], TORCH_TO_O3DMI[p.dtype],
            _vec3(orientation_reference, "orientation_reference"), stream()),
        "orient_normals_to_align_with_direction")
    return _carried(attrs, normals=nrm)


def orient_normals_towards_camera_location(attrs,
                                           camera_location=(0.0, 0.0, 0.0)):
    """PointCloud::OrientNormalsTowardsCameraLocation."""
    p = _positions(attrs)
    nrm = _normals(attrs, p, "No normals in the PointCloud. Call "
                   "EstimateNormals() first.").clone()
    _lib.check(
        _lib.lib().o3dmi_pointcloud_orient_normals_towards_camera_location(
            _lib.ptr(p), _lib.ptr(nrm), p.shape[0], TORCH_TO_O3DMI[p.dtype],
            _vec3(camera_location, "camera_location"), stream()),
        "orient_normals_towards_camera_location")
    return _carried(attrs, normals=nrm)


# ---- segmentation ------------------------------------------------------------------

def cluster_dbscan(attrs, eps, min_points, return_counts=False):
    """PointCloud::ClusterDBSCAN -> Int32 {N} labels (-1 = noise), the labels
    of upstream's sequential loop; with return_counts also (clusters, noise)."""
    p = _positions(attrs)
    n = p.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=p.device)
    clusters, noise = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_pointcloud_cluster_dbscan(
        _lib.ptr(p), n, TORCH_TO_O3DMI[p.dtype], C.c_double(eps),
        int(min_points), _lib.ptr(labels), C.byref(clusters), C.byref(noise),
        stream()), "cluster_dbscan")
    if return_counts:
        return labels, clusters.value, noise.value
    return labels


def segment_plane(attrs, distance_threshold=0.01, ransac_n=3,
                  num_iterations=100, probability=0.99999999, seed=0,
                  return_info=False):
    """PointCloud::SegmentPlane -> (plane Float64 {4} on the cloud's device,
    inliers Int64 {M} ascending); with return_info also a dict(best_iteration,
    iterations_counted, final_break_iteration, fitness, inlier_rmse)."""
    p = _positions(attrs)
    n = p.shape[0]
    inliers = torch.empty(n, dtype=torch.int64, device=p.device)
    plane = (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    m = C.c_int64(0)
    info = _lib.SegmentPlaneInfoC()
    _lib.check(_lib.lib().o3dmi_pointcloud_segment_plane(
        _lib.ptr(p), n, TORCH_TO_O3DMI[p.dtype], C.c_double(distance_threshold),
        int(ransac_n), int(num_iterations), C.c_double(probability),
        C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), plane, _lib.ptr(inliers),
        C.byref(m), C.byref(info), stream()), "segment_plane")
    model = torch.tensor(list(plane), dtype=torch.float64, device=p.device)
    out = inliers[:m.value]
    if return_info:
        return model, out, dict(
            best_iteration=info.best_iteration,
            iterations_counted=info.iterations_counted,
            final_break_iteration=info.final_break_iteration,
            fitness=info.fitness, inlier_rmse=info.inlier_rmse)
    return model, out


def _hull_call(p, index_dtype, call, where):
    """One native call at the bounds V <= n, T <= 2 n - 4, narrowed to the
    counts -> (positions, point indices, triangles)."""
    n = p.shape[0]
    positions = torch.empty((n, 3), dtype=p.dtype, device=p.device)
    indices = torch.empty(n, dtype=index_dtype, device=p.device)
    n_tri = max(2 * n - 4, 0)
    triangles = torch.empty((n_tri, 3), dtype=index_dtype, device=p.device)
    n_v, n_t = C.c_int64(0), C.c_int64(0)
    _lib.check(call(_lib.ptr(positions), _lib.ptr(indices), n,
                    _lib.ptr(triangles), n_tri, TORCH_TO_O3DMI[index_dtype],
                    C.byref(n_v), C.byref(n_t), stream()), where)
    return (positions[:n_v.value], indices[:n_v.value],
            triangles[:n_t.value])


def compute_convex_hull(attrs, joggle_inputs=False):
    """PointCloud::ComputeConvexHull -> the hull as a mesh dict: "positions"
    (bit copies of the hull's points, in ascending point index), "indices"
    Int32 {T,3} and the vertex attribute "point_indices" Int32 {V}. The hull
    is a pure function of the input: triangles are wound counter-clockwise seen
    from outside, rotated to their lowest vertex and sorted by rows (upstream:
    Qhull's traversal order). joggle_inputs=True raises ValueError: Qhull's
    random joggle is not reproduced; degenerate inputs are settled by the eps
    rule of o3dmi_pointcloud_convex_hull instead. A flat cloud raises
    O3DMIError (status 5), as Qhull's QH6154 does upstream."""
    if joggle_inputs:
        raise ValueError("joggle_inputs is not supported: the hull is "
                         "deterministic, degenerate inputs go by the eps rule")
    p = _positions(attrs)
    call = _lib.lib().o3dmi_pointcloud_convex_hull
    positions, indices, triangles = _hull_call(
        p, torch.int32,
        lambda *out: call(_lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype],
                          *out),
        "compute_convex_hull")
    return {"positions": positions, "indices": triangles,
            "point_indices": indices}


def hidden_point_removal(attrs, camera_location, radius):
    """PointCloud::HiddenPointRemoval (Katz et al.) -> (mesh dict of the
    visible points with "positions" (the original rows) and "indices" Int64,
    point indices Int64 {V} ascending). camera_location: 3 numbers or a tensor
    of shape {3}; radius > 0."""
    p = _positions(attrs)
    if isinstance(camera_location, torch.Tensor):
        camera_location = camera_location.detach().to(
            "cpu", torch.float64).reshape(-1).tolist()
    values = [float(e) for e in camera_location]
    if len(values) != 3:
        raise ValueError("camera_location must have shape {3}")
    camera = (C.c_double * 3)(*values)
    call = _lib.lib().o3dmi_pointcloud_hidden_point_removal
    positions, indices, triangles = _hull_call(
        p, torch.int64,
        lambda *out: call(_lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype],
                          camera, C.c_double(float(radius)), *out),
        "hidden_point_removal")
    return {"positions": positions, "indices": triangles}, indices


# ---- oriented bounding volumes -----------------------------------------------------
OBB_METHODS = {"minimal_approx": 0, "pca": 1, "minimal_jylanki": 2}


def _refuse_robust(robust):
    if robust:
        raise ValueError("robust is not supported: Qhull's joggle is not "
                         "reproduced, degenerate inputs go by the hull's eps "
                         "rule")


def _volume_tensors(p, center, rotation, third):
    return (torch.tensor(list(center), dtype=torch.float64).to(p.device,
                                                               p.dtype),
            torch.tensor(list(rotation), dtype=torch.float64).reshape(
                3, 3).to(p.device, p.dtype),
            torch.tensor(list(third), dtype=torch.float64).to(p.device,
                                                              p.dtype))


def get_oriented_bounding_box(attrs, robust=False, method="minimal_approx"):
    """PointCloud::GetOrientedBoundingBox -> dict(center {3}, rotation {3,3},
    extent {3}) as tensors of the cloud's dtype on its device. method:
    "minimal_approx" (upstream's default) or "pca"; "minimal_jylanki" raises
    O3DMIError (status 7): upstream's result depends on a random traversal
    order. robust=True raises ValueError, a flat cloud O3DMIError (status 5).
    The box goes straight into crop(center=, rotation=, extent=)."""
    _refuse_robust(robust)
    if method not in OBB_METHODS:
        raise ValueError("method must be one of %s" % sorted(OBB_METHODS))
    p = _positions(attrs)
    center, rotation, extent = ((C.c_double * 3)(), (C.c_double * 9)(),
                                (C.c_double * 3)())
    _lib.check(_lib.lib().o3dmi_pointcloud_oriented_bounding_box(
        _lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype], OBB_METHODS[method],
        center, rotation, extent, stream()), "get_oriented_bounding_box")
    c, r, e = _volume_tensors(p, center, rotation, extent)
    return {"center": c, "rotation": r, "extent": e}


def get_oriented_bounding_ellipsoid(attrs, robust=False):
    """PointCloud::GetOrientedBoundingEllipsoid (Khachiyan's algorithm on the
    hull's vertices) -> dict(center {3}, rotation {3,3}, radii {3}) as tensors
    of the cloud's dtype on its device."""
    _refuse_robust(robust)
    p = _positions(attrs)
    center, rotation, radii = ((C.c_double * 3)(), (C.c_double * 9)(),
                               (C.c_double * 3)())
    _lib.check(_lib.lib().o3dmi_pointcloud_oriented_bounding_ellipsoid(
        _lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype], center, rotation,
        radii, None, stream()), "get_oriented_bounding_ellipsoid")
    c, r, e = _volume_tensors(p, center, rotation, radii)
    return {"center": c, "rotation": r, "radii": e}


_BOX_CORNERS = ((-1, -1, -1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1),
                (1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1))


def box_points(box):
    """OrientedBoundingBox::GetBoxPoints -> {8,3} in upstream's corner order
    (geometry/BoundingVolume.cpp:190-204)."""
    c, r, e = box["center"], box["rotation"], box["extent"]
    axes = r * (e / 2)[None, :]  # column k = R (extent_k / 2) e_k
    signs = torch.tensor(_BOX_CORNERS, dtype=c.dtype, device=c.device)
    return c[None, :] + signs @ axes.T


def ellipsoid_points(ellipsoid):
    """OrientedBoundingEllipsoid::GetEllipsoidPoints -> {6,3}: center +/- each
    axis scaled by its radius, the x pair first
    (geometry/BoundingVolume.cpp:98-111)."""
    c, r, e = ellipsoid["center"], ellipsoid["rotation"], ellipsoid["radii"]
    axes = (r * e[None, :]).T  # row k = R radii_k e_k
    return torch.stack([c + s * axes[k] for k in range(3) for s in (1, -1)])
