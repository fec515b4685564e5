"""Mirror of the rigid half of open3d.t.pipelines.slac on the HIP backend
(tests and tools; a binding calls the C ABI directly).

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
