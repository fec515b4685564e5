"""Mirror of open3d.t.pipelines.slac on the HIP backend: the rigid and the
non-rigid optimizer and ControlGrid (tests and tools; a binding calls the C ABI directly).

Fragments are (positions, normals) float32 CUDA tensors in memory; the
reference takes file names and caches .npy / .ply files in slac_folder.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np
import torch

from . import _lib
from .core import stream as _stream

SINGULAR = 5  # O3DMI_ERR_SINGULAR


@dataclass
class SLACOptimizerParams:
    """t/pipelines/slac/SLACOptimizer.h:66-88 (voxel_size belongs to the
    preprocessing, which is the caller's)."""
    max_iterations: int = 5
    voxel_size: float = 0.05
    distance_threshold: float = 0.07
    fitness_threshold: float = 0.3
    regularizer_weight: float = 1.0


@dataclass
class PoseGraph:
    """nodes: 4x4 float64 poses; edges: (source, target, transformation)."""
    nodes: List[np.ndarray] = field(default_factory=list)
    edges: List[Tuple[int, int, np.ndarray]] = field(default_factory=list)


def _f32(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and \
        t.shape[1] == 3, "fragments are {n,3} Float32 CUDA tensors"
    return t.contiguous()


def _T(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(4, 4))


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def get_correspondence_set_for_point_cloud_pair(i, j, positions_i, positions_j,
                                                T_i, T_j, T_ij,
                                                distance_threshold,
                                                fitness_threshold,
                                                return_info=False):
    """GetCorrespondenceSetForPointCloudPair: the {C,2} int64 set, empty when
    the pair is pruned. return_info adds dict(n_corres, n_inliers,
    inlier_ratio, kept)."""
    pi, pj = _f32(positions_i), _f32(positions_j)
    out = torch.empty((pi.shape[0], 2), dtype=torch.int64, device=pi.device)
    c, inl = C.c_int64(0), C.c_int64(0)
    ratio, kept = C.c_float(0), C.c_int(0)
    T_i, T_j, T_ij = _T(T_i), _T(T_j), _T(T_ij)
    _lib.check(_lib.lib().o3dmi_slac_correspondence_set(
        _lib.ptr(pi), pi.shape[0], _lib.ptr(pj), pj.shape[0], int(i), int(j),
        _lib.f64p(T_i), _lib.f64p(T_j), _lib.f64p(T_ij),
        float(distance_threshold), float(fitness_threshold), _lib.ptr(out),
        C.byref(c), C.byref(inl), C.byref(ratio), C.byref(kept), _stream()),
        "slac_correspondence_set")
    corres = out[:c.value if kept.value else 0]
    if return_info:
        return corres, dict(n_corres=c.value, n_inliers=inl.value,
                            inlier_ratio=np.float32(ratio.value),
                            kept=bool(kept.value), all_pairs=out[:c.value])
    return corres


def fill_in_rigid_alignment_term(AtA, Atb, residual, Ti_ps, Tj_qs,
                                 Ri_normal_ps, i, j, threshold):
    """kernel::FillInRigidAlignmentTerm: adds the edge's 12x12 block, rhs and
    residual to the float32 AtA {6N,6N}, Atb {6N}, residual {1} in place."""
    for t in (AtA, Atb, residual):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert AtA.dim() == 2 and AtA.shape[0] == AtA.shape[1] == Atb.numel()
    p, q, n = _f32(Ti_ps), _f32(Tj_qs), _f32(Ri_normal_ps)
    assert p.shape == q.shape == n.shape, "input length mismatch"
    _lib.check(_lib.lib().o3dmi_fill_in_rigid_alignment_term(
        _lib.ptr(AtA), _lib.ptr(Atb), _lib.ptr(residual), AtA.shape[0],
        _lib.ptr(p), _lib.ptr(q), _lib.ptr(n), p.shape[0], int(i), int(j),
        float(threshold), _stream()), "fill_in_rigid_alignment_term")


def rigid_terms(fragments, poses, edges, correspondences, threshold,
                out=None):
    """o3dmi_slac_rigid_terms: the {E,29} float64 sums of all edges in one
    launch. fragments: list of (positions, normals); poses: N 4x4 float64;
    edges: list of (i, j); correspondences: list of {C,2} int64 tensors."""
    pos = [_f32(f[0]) for f in fragments]
    nrm = [_f32(f[1]) for f in fragments]
    cor = [c.contiguous() for c in correspondences]
    for c in cor:
        assert c.is_cuda and c.dtype == torch.int64
    E = len(edges)
    if out is None:
        out = torch.zeros((E, 29), dtype=torch.float64, device=pos[0].device)
    sizes = (C.c_int64 * len(pos))(*[p.shape[0] for p in pos])
    ed = (C.c_int32 * (2 * E))(*[int(v) for e in edges for v in e[:2]])
    counts = (C.c_int64 * E)(*[c.shape[0] for c in cor])
    P = np.ascontiguousarray(np.stack([_T(T) for T in poses]))
    _lib.check(_lib.lib().o3dmi_slac_rigid_terms(
        _ptr_array(pos), _ptr_array(nrm), sizes, len(pos), ed,
        _ptr_array(cor), counts, E, _lib.f64p(P), float(threshold),
        _lib.ptr(out), _stream()), "slac_rigid_terms")
    return out


def rigid_optimize_raw(fragments, nodes, edges, params):
    """o3dmi_slac_rigid_optimize without the status check: (status, poses
    {N,4,4} as the call left them, info)."""
    pos = [_f32(f[0]) for f in fragments]
    nrm = [_f32(f[1]) for f in fragments]
    N, E = len(nodes), len(edges)
    assert N == len(pos), "one fragment per node"
    sizes = (C.c_int64 * N)(*[p.shape[0] for p in pos])
    P = np.ascontiguousarray(np.stack([_T(T) for T in nodes]))
    ed = (C.c_int32 * max(2 * E, 1))(*[int(v) for e in edges for v in e[:2]])
    Tij = np.ascontiguousarray(
        np.stack([_T(e[2]) for e in edges]) if E else np.zeros((1, 4, 4)))
    iters = max(int(params.max_iterations), 0)
    losses = np.zeros(max(iters, 1), np.float64)
    kept = (C.c_int32 * max(E, 1))()
    n_corres = (C.c_int64 * max(E, 1))()
    n_inliers = (C.c_int64 * max(E, 1))()
    status = _lib.lib().o3dmi_slac_rigid_optimize(
        _ptr_array(pos), _ptr_array(nrm), sizes, N, _lib.f64p(P), ed,
        _lib.f64p(Tij), E, int(params.max_iterations),
        float(params.distance_threshold), float(params.fitness_threshold),
        _lib.f64p(losses), kept, n_corres, n_inliers, _stream())
    return status, P, dict(losses=losses[:iters].copy(),
                           kept=[bool(v) for v in kept[:E]],
                           n_corres=list(n_corres[:E]),
                           n_inliers=list(n_inliers[:E]))


def run_rigid_optimizer_for_fragments(fragments, pose_graph, params=None,
                                      return_info=False):
    """RunRigidOptimizerForFragments: a PoseGraph with the updated node poses
    (edges unchanged). return_info adds dict(losses, kept, n_corres,
    n_inliers)."""
    params = params or SLACOptimizerParams()
    status, P, info = rigid_optimize_raw(fragments, pose_graph.nodes,
                                         pose_graph.edges, params)
    _lib.check(status, "slac_rigid_optimize")
    out = PoseGraph([P[k].copy() for k in range(P.shape[0])],
                    list(pose_graph.edges))
    return (out, info) if return_info else out


# ---- ControlGrid (t/pipelines/slac/ControlGrid.{h,cpp}) ---------------------

def _rows(t, name, cols=3, dtype=torch.float32):
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype \
        and t.dim() == 2 and t.shape[1] == cols, \
        "%s must be a {n,%d} %s device tensor" % (name, cols, dtype)
    return t.contiguous()


def _frame_args(depth, intrinsic, extrinsic):
    from .core import host_mat
    from .geometry import _image
    depth = _image(depth, "depth", 1)
    return (depth, host_mat(intrinsic, (3, 3), "intrinsic"),
            host_mat(extrinsic, (4, 4), "extrinsic"))


def create_from_rgbd_image(depth, color, intrinsic, extrinsic,
                           depth_scale=1000.0, depth_max=3.0):
    """PointCloud::CreateFromDepthImage / CreateFromRGBDImage at stride 1:
    (positions, colors or None) in the row-major order of the pixels. A UInt8
    colour image is scaled by 1/255 first (Image::To)."""
    from .core import TORCH_TO_O3DMI
    from .odometry import to_float
    depth, K, T = _frame_args(depth, intrinsic, extrinsic)
    rows, cols = depth.shape
    pts = torch.empty((rows * cols, 3), dtype=torch.float32, device="cuda")
    image_colors = cols_out = None
    if color is not None:
        image_colors = color if color.dtype == torch.float32 else \
            to_float(color.contiguous(), 1.0 / 255)
        cols_out = torch.empty_like(pts)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().o3dmi_unproject(
        _lib.ptr(depth), TORCH_TO_O3DMI[depth.dtype], rows, cols,
        _lib.ptr(image_colors), _lib.ptr(pts), _lib.ptr(cols_out),
        _lib.ptr(count), _lib.f64p(K), _lib.f64p(T), float(depth_scale),
        float(depth_max), 1, _stream()), "unproject")
    n = int(count.item())
    return pts[:n], (cols_out[:n] if cols_out is not None else None)


def project_to_depth_image(positions, width, height, intrinsic, extrinsic,
                           depth_scale=1000.0, depth_max=3.0):
    """PointCloud::ProjectToDepthImage: {height,width} Float32."""
    from .core import host_mat
    p = _rows(positions, "positions")
    K = host_mat(intrinsic, (3, 3), "intrinsic")
    T = host_mat(extrinsic, (4, 4), "extrinsic")
    depth = torch.empty((height, width), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().o3dmi_project_to_depth_image(
        _lib.ptr(p), p.shape[0], int(height), int(width), _lib.f64p(K),
        _lib.f64p(T), float(depth_scale), float(depth_max), _lib.ptr(depth),
        _stream()), "project_to_depth_image")
    return depth


def project_to_rgbd_image(positions, colors, width, height, intrinsic,
                          extrinsic, depth_scale=1000.0, depth_max=3.0):
    """PointCloud::ProjectToRGBDImage: (depth {height,width}, color
    {height,width,3}), Float32."""
    from .core import host_mat
    p, c = _rows(positions, "positions"), _rows(colors, "colors")
    assert p.shape == c.shape, "one colour per point"
    K = host_mat(intrinsic, (3, 3), "intrinsic")
    T = host_mat(extrinsic, (4, 4), "extrinsic")
    depth = torch.empty((height, width), dtype=torch.float32, device="cuda")
    color = torch.empty((height, width, 3), dtype=torch.float32,
                        device="cuda")
    _lib.check(_lib.lib().o3dmi_project_to_rgbd_image(
        _lib.ptr(p), _lib.ptr(c), p.shape[0], int(height), int(width),
        _lib.f64p(K), _lib.f64p(T), float(depth_scale), float(depth_max),
        _lib.ptr(depth), _lib.ptr(color), _stream()),
        "project_to_rgbd_image")
    return depth, color


@dataclass
class ParameterizedCloud:
    """The point cloud ControlGrid.parameterize returns: the attributes
    Grid8NbIndices, Grid8NbVertexInterpRatios and Grid8NbNormalInterpRatios
    beside positions / normals / colors (None where the input had none)."""
    positions: torch.Tensor
    normals: torch.Tensor
    colors: torch.Tensor
    Grid8NbIndices: torch.Tensor
    Grid8NbVertexInterpRatios: torch.Tensor
    Grid8NbNormalInterpRatios: torch.Tensor


class ControlGrid:
    """Mirror of o3d.t.pipelines.slac.control_grid. Clouds are {n,3} Float32
    device tensors; images as in VoxelBlockGrid."""

    def __init__(self, grid_size, grid_count=1000, keys=None, values=None):
        h = C.c_void_p()
        if keys is not None:
            k = _rows(keys, "keys", 3, torch.int32)
            v = _rows(values, "values")
            assert k.shape == v.shape, "one value per key"
            _lib.check(_lib.lib().o3dmi_control_grid_create_from(
                float(grid_size), _lib.ptr(k), _lib.ptr(v), k.shape[0],
                _stream(), C.byref(h)), "ControlGrid")
        else:
            _lib.check(_lib.lib().o3dmi_control_grid_create(
                float(grid_size), int(grid_count), _stream(), C.byref(h)),
                "ControlGrid")
        self._g = h
        self.grid_size = float(grid_size)

    def __del__(self):
        try:
            if getattr(self, "_g", None):
                _lib.lib().o3dmi_control_grid_destroy(self._g)
                self._g = None
        except Exception:
            pass

    def touch(self, positions):
        p = _rows(positions, "positions")
        _lib.check(_lib.lib().o3dmi_control_grid_touch(
            self._g, _lib.ptr(p), p.shape[0], _stream()), "ControlGrid.touch")

    def compactify(self):
        _lib.check(_lib.lib().o3dmi_control_grid_compactify(
            self._g, _stream()), "ControlGrid.compactify")

    def size(self):
        n = C.c_int64(0)
        _lib.check(_lib.lib().o3dmi_control_grid_size(
            self._g, _stream(), C.byref(n)), "ControlGrid.size")
        return int(n.value)

    def get_anchor_idx(self):
        return int(_lib.lib().o3dmi_control_grid_anchor_idx(self._g))

    def get_hashmap(self):
        from .geometry import HashMapView
        return HashMapView(
            C.c_void_p(_lib.lib().o3dmi_control_grid_hashmap(self._g)), self)

    def get_init_positions(self):
        cap = self.get_hashmap().capacity()
        out = torch.empty((cap, 3), dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().o3dmi_control_grid_init_positions(
            self._g, _lib.ptr(out), _stream()),
            "ControlGrid.get_init_positions")
        return out

    def get_curr_positions(self):
        """The value buffer itself (writable); a touch or a compactify moves
        it, so take it again afterwards."""
        from .core import tensor_from_ptr
        p = _lib.lib().o3dmi_control_grid_curr_positions(self._g)
        return tensor_from_ptr(p, (self.get_hashmap().capacity(), 3),
                               _lib.F32, self)

    def get_neighbor_grid_map(self):
        """(active buffer indices {n}, neighbour indices {n,6}, masks {n,6}),
        neighbours in the order -x +x -y +y -z +z."""
        cap = self.get_hashmap().capacity()
        active = torch.empty(cap, dtype=torch.int32, device="cuda")
        nb = torch.empty((cap, 6), dtype=torch.int32, device="cuda")
        masks = torch.empty((cap, 6), dtype=torch.bool, device="cuda")
        n = C.c_int64(0)
        _lib.check(_lib.lib().o3dmi_control_grid_neighbor_grid_map(
            self._g, _lib.ptr(active), _lib.ptr(nb), _lib.ptr(masks),
            C.byref(n), _stream()), "ControlGrid.get_neighbor_grid_map")
        return active[:n.value], nb[:n.value], masks[:n.value]

    def parameterize(self, positions, normals=None, colors=None):
        p = _rows(positions, "positions")
        nm = _rows(normals, "normals") if normals is not None else None
        cl = _rows(colors, "colors") if colors is not None else None
        n = p.shape[0]

        def new(cols, dtype=torch.float32):
            return torch.empty((n, cols), dtype=dtype, device="cuda")
        op, idx, vr = new(3), new(8, torch.int32), new(8)
        on = new(3) if nm is not None else None
        nr = new(8) if nm is not None else None
        oc = new(3) if cl is not None else None
        m = C.c_int64(0)
        _lib.check(_lib.lib().o3dmi_control_grid_parameterize(
            self._g, _lib.ptr(p), _lib.ptr(nm), _lib.ptr(cl), n, n,
            _lib.ptr(op), _lib.ptr(on), _lib.ptr(oc), _lib.ptr(idx),
            _lib.ptr(vr), _lib.ptr(nr), C.byref(m), _stream()),
            "ControlGrid.parameterize")

        def cut(t):
            return t[:m.value] if t is not None else None
        return ParameterizedCloud(cut(op), cut(on), cut(oc), cut(idx), cut(vr),
                                  cut(nr))

    def deform_raw(self, cloud, out_positions, out_normals=None):
        """o3dmi_control_grid_deform into caller-provided outputs; returns the
        status instead of raising."""
        idx = _rows(cloud.Grid8NbIndices, "Grid8NbIndices", 8, torch.int32)
        vr = _rows(cloud.Grid8NbVertexInterpRatios, "vertex ratios", 8)
        nr = cloud.Grid8NbNormalInterpRatios
        if out_normals is None:
            nr = None
        return _lib.lib().o3dmi_control_grid_deform(
            self._g, _lib.ptr(idx), _lib.ptr(vr), _lib.ptr(nr), idx.shape[0],
            _lib.ptr(out_positions), _lib.ptr(out_normals), _stream())

    def deform(self, *args, **kwargs):
        """deform(cloud) -> (positions, normals, colors);
        deform(depth, intrinsic, extrinsic, depth_scale, depth_max) -> depth;
        deform((depth, color), intrinsic, extrinsic, depth_scale, depth_max)
        -> (depth, color). Images come back as Float32."""
        first = args[0]
        if isinstance(first, ParameterizedCloud):
            return self._deform_cloud(first)
        if isinstance(first, (tuple, list)):
            return self._deform_rgbd(first[0], first[1], *args[1:], **kwargs)
        return self._deform_depth(*args, **kwargs)

    def _deform_cloud(self, cloud):
        n = cloud.Grid8NbIndices.shape[0]
        pos = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        nrm = torch.empty_like(pos) \
            if cloud.Grid8NbNormalInterpRatios is not None else None
        _lib.check(self.deform_raw(cloud, pos, nrm), "ControlGrid.deform")
        return pos, nrm, cloud.colors

    def _deform_depth(self, depth, intrinsic, extrinsic, depth_scale=1000.0,
                      depth_max=3.0):
        from .core import TORCH_TO_O3DMI
        depth, K, T = _frame_args(depth, intrinsic, extrinsic)
        rows, cols = depth.shape
        out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().o3dmi_control_grid_deform_depth_image(
            self._g, _lib.ptr(depth), TORCH_TO_O3DMI[depth.dtype], rows, cols,
            _lib.f64p(K), _lib.f64p(T), float(depth_scale), float(depth_max),
            _lib.ptr(out), _stream()), "ControlGrid.deform")
        return out

    def _deform_rgbd(self, depth, color, intrinsic, extrinsic,
                     depth_scale=1000.0, depth_max=3.0):
        from .core import TORCH_TO_O3DMI
        from .geometry import _image
        depth, K, T = _frame_args(depth, intrinsic, extrinsic)
        color = _image(color, "color", 3)
        rows, cols = depth.shape
        assert color.shape[:2] == (rows, cols), "depth / colour size mismatch"
        out_d = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
        out_c = torch.empty((rows, cols, 3), dtype=torch.float32,
                            device="cuda")
        _lib.check(_lib.lib().o3dmi_control_grid_deform_rgbd_image(
            self._g, _lib.ptr(depth), TORCH_TO_O3DMI[depth.dtype],
            _lib.ptr(color), TORCH_TO_O3DMI[color.dtype], rows, cols,
            _lib.f64p(K), _lib.f64p(T), float(depth_scale), float(depth_max),
            _lib.ptr(out_d), _lib.ptr(out_c), _stream()),
            "ControlGrid.deform")
        return out_d, out_c

    def deform_seam_by_seam(self, depth, color, intrinsic, extrinsic,
                            depth_scale=1000.0, depth_max=3.0):
        """The reference's chain for an image: CreateFrom{Depth,RGBD}Image ->
        Parameterize -> Deform -> ProjectTo{Depth,RGBD}Image. Same bits as
        deform(); kept callable for checks and measurements."""
        rows, cols = depth.shape[:2]
        pts, cl = create_from_rgbd_image(depth, color, intrinsic, extrinsic,
                                         depth_scale, depth_max)
        pos, _, cl = self._deform_cloud(self.parameterize(pts, colors=cl))
        if color is None:
            return project_to_depth_image(pos, cols, rows, intrinsic,
                                          extrinsic, depth_scale, depth_max)
        return project_to_rgbd_image(pos, cl, cols, rows, intrinsic,
                                     extrinsic, depth_scale, depth_max)


# ---- the non-rigid optimizer (SLACOptimizer.cpp:253-367) --------------------

def _system(AtA, Atb, residual):
    for t in (AtA, Atb, residual):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert AtA.dim() == 2 and AtA.shape[0] == AtA.shape[1] == Atb.numel()


def fill_in_slac_alignment_term_raw(AtA, Atb, residual, Ti_Cps, Tj_Cqs,
                                    Cnormal_ps, Ri_Cnormal_ps,
                                    RjT_Ri_Cnormal_ps, cgrid_idx_ps,
                                    cgrid_idx_qs, cgrid_ratio_ps,
                                    cgrid_ratio_qs, i, j, n_frags, threshold):
    """o3dmi_fill_in_slac_alignment_term; returns the status."""
    _system(AtA, Atb, residual)
    rows = [_f32(t) for t in (Ti_Cps, Tj_Cqs, Cnormal_ps, Ri_Cnormal_ps,
                              RjT_Ri_Cnormal_ps)]
    ip = _rows(cgrid_idx_ps, "cgrid_idx_ps", 8, torch.int32)
    iq = _rows(cgrid_idx_qs, "cgrid_idx_qs", 8, torch.int32)
    rp = _rows(cgrid_ratio_ps, "cgrid_ratio_ps", 8)
    rq = _rows(cgrid_ratio_qs, "cgrid_ratio_qs", 8)
    n = rows[0].shape[0]
    assert all(t.shape[0] == n for t in rows + [ip, iq, rp, rq]), \
        "input length mismatch"
    return _lib.lib().o3dmi_fill_in_slac_alignment_term(
        _lib.ptr(AtA), _lib.ptr(Atb), _lib.ptr(residual), AtA.shape[0],
        *[_lib.ptr(t) for t in rows], _lib.ptr(ip), _lib.ptr(iq),
        _lib.ptr(rp), _lib.ptr(rq), n, int(i), int(j), int(n_frags),
        float(threshold), _stream())


def fill_in_slac_alignment_term(*args):
    """kernel::FillInSLACAlignmentTerm: adds an edge's terms to the float32
    AtA {n,n}, Atb {n}, residual {1} in place. The ratio arrays follow their
    index arrays: (.., idx_ps, idx_qs, ratio_ps, ratio_qs, i, j, n_frags,
    threshold)."""
    _lib.check(fill_in_slac_alignment_term_raw(*args),
               "fill_in_slac_alignment_term")


def fill_in_slac_regularizer_term_raw(AtA, Atb, residual, grid_idx,
                                      grid_nbs_idx, grid_nbs_mask,
                                      positions_init, positions_curr, weight,
                                      n_frags, anchor_idx):
    """o3dmi_fill_in_slac_regularizer_term; returns the status."""
    _system(AtA, Atb, residual)
    gi = grid_idx.contiguous()
    assert gi.is_cuda and gi.dtype == torch.int32 and gi.dim() == 1
    nb = _rows(grid_nbs_idx, "grid_nbs_idx", 6, torch.int32)
    mk = _rows(grid_nbs_mask, "grid_nbs_mask", 6, torch.bool)
    p0, p1 = _rows(positions_init, "init"), _rows(positions_curr, "curr")
    assert nb.shape[0] == mk.shape[0] == gi.shape[0] and p0.shape == p1.shape
    return _lib.lib().o3dmi_fill_in_slac_regularizer_term(
        _lib.ptr(AtA), _lib.ptr(Atb), _lib.ptr(residual), AtA.shape[0],
        _lib.ptr(gi), _lib.ptr(nb), _lib.ptr(mk), gi.shape[0], _lib.ptr(p0),
        _lib.ptr(p1), p0.shape[0], float(weight), int(n_frags),
        int(anchor_idx), _stream())


def fill_in_slac_regularizer_term(*args):
    """kernel::FillInSLACRegularizerTerm on GetNeighborGridMap's output."""
    _lib.check(fill_in_slac_regularizer_term_raw(*args),
               "fill_in_slac_regularizer_term")


def solve_spd_raw(A, b):
    """o3dmi_slac_solve_spd in place on a float64 {n,n} lower triangle and
    {n} right-hand side; returns the status."""
    for t in (A, b):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    return _lib.lib().o3dmi_slac_solve_spd(_lib.ptr(A), _lib.ptr(b),
                                           b.numel(), _stream())


def solve_spd(A, b):
    """x = solve(A, b) for symmetric positive definite A (only the lower
    triangle is read); neither input is modified."""
    L, x = A.clone(), b.clone()
    _lib.check(solve_spd_raw(L, x), "slac_solve_spd")
    return x


def slac_optimize_raw(fragments, nodes, edges, params, control_grid):
    """o3dmi_slac_optimize without the status check: (status, poses {N,4,4}
    as the call left them, info). The grid is updated in place."""
    pos = [_f32(f[0]) for f in fragments]
    nrm = [_f32(f[1]) for f in fragments]
    N, E = len(nodes), len(edges)
    assert N == len(pos), "one fragment per node"
    sizes = (C.c_int64 * N)(*[p.shape[0] for p in pos])
    P = np.ascontiguousarray(np.stack([_T(T) for T in nodes]))
    ed = (C.c_int32 * max(2 * E, 1))(*[int(v) for e in edges for v in e[:2]])
    Tij = np.ascontiguousarray(
        np.stack([_T(e[2]) for e in edges]) if E else np.zeros((1, 4, 4)))
    iters = max(int(params.max_iterations), 0)
    align = np.zeros(max(iters, 1), np.float64)
    reg = np.zeros(max(iters, 1), np.float64)
    kept = (C.c_int32 * max(E, 1))()
    n_corres = (C.c_int64 * max(E, 1))()
    n_inliers = (C.c_int64 * max(E, 1))()
    skipped = C.c_int64(0)
    status = _lib.lib().o3dmi_slac_optimize(
        _ptr_array(pos), _ptr_array(nrm), sizes, N, _lib.f64p(P), ed,
        _lib.f64p(Tij), E, control_grid._g, int(params.max_iterations),
        float(params.distance_threshold), float(params.fitness_threshold),
        float(params.regularizer_weight), _lib.f64p(align), _lib.f64p(reg),
        kept, n_corres, n_inliers, C.byref(skipped), _stream())
    return status, P, dict(alignment_losses=align[:iters].copy(),
                           regularizer_losses=reg[:iters].copy(),
                           kept=[bool(v) for v in kept[:E]],
                           n_corres=list(n_corres[:E]),
                           n_inliers=list(n_inliers[:E]),
                           skipped=int(skipped.value))


def run_slac_optimizer_for_fragments(fragments, pose_graph, params=None,
                                     control_grid=None, return_info=False):
    """RunSLACOptimizerForFragments: (PoseGraph with the updated node poses,
    ControlGrid). control_grid None: the reference's ControlGrid(3.0 / 8,
    8000), touched with every fragment; a grid that has nodes is continued.
    return_info adds dict(alignment_losses, regularizer_losses, kept,
    n_corres, n_inliers, skipped)."""
    params = params or SLACOptimizerParams()
    grid = control_grid if control_grid is not None else \
        ControlGrid(3.0 / 8, 8000)
    status, P, info = slac_optimize_raw(fragments, pose_graph.nodes,
                                        pose_graph.edges, params, grid)
    _lib.check(status, "slac_optimize")
    out = PoseGraph([P[k].copy() for k in range(P.shape[0])],
                    list(pose_graph.edges))
    return (out, grid, info) if return_info else (out, grid)


def preprocess_point_cloud(positions, normals=None, voxel_size=0.05,
                           apply_outlier_mask=False):
    """The per-fragment step of PreprocessPointClouds (SLACOptimizer.cpp:
    47-57): voxel_size > 0: VoxelDownSample -> RemoveStatisticalOutliers(20,
    2.0) -> EstimateNormals (KNN, 30); otherwise the filter, then
    EstimateNormals only when `normals` is None. The reference computes the
    filter and drops its result; apply_outlier_mask=True applies it.
    -> (positions, normals)."""
    p = positions.contiguous()
    assert p.is_cuda and p.dim() == 2 and p.shape[1] == 3
    nrm = None if normals is None else normals.contiguous()
    out_p = torch.empty_like(p)
    out_n = torch.empty_like(p)
    m = C.c_int64(0)
    dtype = _lib.F64 if p.dtype == torch.float64 else _lib.F32
    _lib.check(_lib.lib().o3dmi_slac_preprocess_point_cloud(
        _lib.ptr(p), _lib.ptr(nrm), p.shape[0], dtype,
        C.c_double(voxel_size), int(bool(apply_outlier_mask)),
        _lib.ptr(out_p), _lib.ptr(out_n), C.byref(m), _stream()),
        "slac_preprocess_point_cloud")
    return out_p[:m.value], out_n[:m.value]
