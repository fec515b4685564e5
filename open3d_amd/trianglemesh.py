"""Mirror of t::geometry::TriangleMesh's normal, area, selection and
connectivity methods (t/geometry/TriangleMesh.cpp:198-404, 1221-1452,
1826-1864), of legacy ClusterConnectedTriangles (geometry/TriangleMesh.cpp:
1459-1528), of SamplePointsUniformly and ComputeMetrics (t/geometry/
TriangleMesh.cpp:1866-1967), of RaycastingScene's closest-point and ray
queries for one mesh (MeshBVH, create_rays_pinhole) and of the legacy clean-up,
smoothing and clustering methods (RemoveDuplicatedVertices / Triangles,
RemoveDegenerateTriangles, ComputeAdjacencyList, FilterSharpen, FilterSmooth*,
SimplifyVertexClustering; geometry/TriangleMesh.cpp:153-440, 680-860,
TriangleMeshSimplification.cpp:72-244) and of the legacy topology and
intersection queries (EulerPoincareCharacteristic, IsEdgeManifold,
GetNonManifoldVertices / IsVertexManifold, IsOrientable / OrientTriangles,
GetSelfIntersectingTriangles / IsSelfIntersecting, IsIntersecting,
IsWatertight, GetVolume; geometry/TriangleMesh.cpp:1016-1135, 1212-1246,
1272-1457), of legacy SubdivideMidpoint / SubdivideLoop (geometry/
TriangleMeshSubdivide.cpp) and of ClipPlane / SlicePlane (t/geometry/
TriangleMesh.cpp:649-716; upstream: VTK on a host copy, here pinned rules on
the device), of ComputeConvexHull (:644; upstream: Qhull on a host copy) and
of GetOrientedBoundingBox / GetOrientedBoundingEllipsoid on the HIP backend.

A mesh is the dict VoxelBlockGrid.extract_triangle_mesh returns: "positions"
({V,3} Float32 or Float64) and "indices" ({M,3} Int32 or Int64) on the device,
further vertex attributes under their own names ("normals", "colors", ...)
and triangle attributes under a "triangle_" prefix ("triangle_normals",
"triangle_areas", ...). Every function returns a new dict; the input is left
as it was.
"""
import ctypes as C

import torch

from . import _lib
from . import pointcloud as _pc
from .core import TORCH_TO_O3DMI, require_cuda, stream

TRIANGLE_PREFIX = "triangle_"


def _positions(mesh):
    if "positions" not in mesh:
        raise ValueError('a mesh needs "positions"')
    p = require_cuda(mesh["positions"], "positions")
    if p.dim() != 2 or p.shape[1] != 3 or p.dtype not in (torch.float32,
                                                          torch.float64):
        raise ValueError("positions must be {V,3} Float32 or Float64")
    return p


def _indices(mesh, p):
    t = mesh.get("indices")
    if t is None:
        return torch.empty((0, 3), dtype=torch.int64, device=p.device)
    t = require_cuda(t, "indices")
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype not in (torch.int32,
                                                          torch.int64):
        raise ValueError("indices must be {M,3} Int32 or Int64")
    return t


def _mesh_args(mesh):
    """-> (positions, indices, the six leading arguments of a mesh call)."""
    p = _positions(mesh)
    t = _indices(mesh, p)
    return p, t, (_lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype],
                  _lib.ptr(t), t.shape[0], TORCH_TO_O3DMI[t.dtype])


def _index_args(p, t):
    return (_lib.ptr(t), t.shape[0], TORCH_TO_O3DMI[t.dtype], p.shape[0])


def _split(mesh):
    """-> (vertex attributes, triangle attributes with "indices")."""
    vertex, triangle = {}, {}
    for name, value in mesh.items():
        if name == "indices" or name.startswith(TRIANGLE_PREFIX):
            triangle[name] = value
        else:
            vertex[name] = value
    return vertex, triangle


def _normalize(t):
    if t.shape[0]:
        _lib.check(_lib.lib().o3dmi_trianglemesh_normalize_normals(
            _lib.ptr(t), t.shape[0], TORCH_TO_O3DMI[t.dtype], stream()),
            "normalize_normals")
    return t


def normalize_normals(mesh):
    """TriangleMesh::NormalizeNormals: the vertex and the triangle normals the
    mesh has, by upstream's mesh rule (a row whose x is NaN stays as it is)."""
    out = dict(mesh)
    for name in ("normals", TRIANGLE_PREFIX + "normals"):
        if name in out:
            out[name] = _normalize(
                require_cuda(out[name], name).contiguous().clone())
    return out


def compute_triangle_normals(mesh, normalized=True):
    """TriangleMesh::ComputeTriangleNormals -> mesh with "triangle_normals"
    (and, when normalized, every normal of the mesh normalised, as
    upstream)."""
    p, t, args = _mesh_args(mesh)
    out = dict(mesh)
    if p.shape[0] == 0 or "indices" not in mesh:
        return out
    normals = torch.empty((t.shape[0], 3), dtype=p.dtype, device=p.device)
    _lib.check(_lib.lib().o3dmi_trianglemesh_compute_triangle_normals(
        *args, _lib.ptr(normals), stream()), "compute_triangle_normals")
    out[TRIANGLE_PREFIX + "normals"] = normals
    return normalize_normals(out) if normalized else out


def compute_vertex_normals(mesh, normalized=True):
    """TriangleMesh::ComputeVertexNormals -> mesh with "triangle_normals" and
    "normals": the sum of upstream's CPU loop, bit for bit."""
    p, t, args = _mesh_args(mesh)
    out = dict(mesh)
    if p.shape[0] == 0 or "indices" not in mesh:
        return out
    tn = torch.empty((t.shape[0], 3), dtype=p.dtype, device=p.device)
    vn = torch.empty((p.shape[0], 3), dtype=p.dtype, device=p.device)
    _lib.check(_lib.lib().o3dmi_trianglemesh_vertex_normals(
        *args, _lib.ptr(tn), _lib.ptr(vn), 0, stream()),
        "compute_vertex_normals")
    out[TRIANGLE_PREFIX + "normals"] = tn
    out["normals"] = vn
    return normalize_normals(out) if normalized else out


def _areas(mesh):
    p, t, args = _mesh_args(mesh)
    areas = torch.empty(t.shape[0], dtype=p.dtype, device=p.device)
    _lib.check(_lib.lib().o3dmi_trianglemesh_compute_triangle_areas(
        *args, _lib.ptr(areas), stream()), "compute_triangle_areas")
    return areas


def compute_triangle_areas(mesh):
    """TriangleMesh::ComputeTriangleAreas -> mesh with "triangle_areas" ({0}
    for a mesh without triangles; areas the mesh already has are kept)."""
    out = dict(mesh)
    if _positions(mesh).shape[0] == 0 or TRIANGLE_PREFIX + "areas" in mesh:
        return out
    out[TRIANGLE_PREFIX + "areas"] = _areas(mesh)
    return out


def get_surface_area(mesh):
    """TriangleMesh::GetSurfaceArea as a float64 sum in a fixed order."""
    _, _, args = _mesh_args(mesh)
    area = C.c_double(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_surface_area(
        *args, C.byref(area), stream()), "get_surface_area")
    return area.value


def _select_rows(rows, mask8):
    """Stable compaction of equally long attribute tensors by a uint8 mask
    (o3dmi_pointcloud_select_by_mask, up to MAX_ATTRS attributes a launch)."""
    names = list(rows)
    n = mask8.shape[0]
    out = {}
    for g in range(0, len(names), _pc.MAX_ATTRS):
        group = names[g:g + _pc.MAX_ATTRS]
        ins = [require_cuda(rows[k], k).contiguous() for k in group]
        for k, t in zip(group, ins):
            if t.dim() < 1 or t.shape[0] != n:
                raise ValueError("attribute %r must have %d rows" % (k, n))
        outs = [torch.empty_like(t) for t in ins]
        m = C.c_int64(0)
        a_in, widths, a_out = _pc._tables(ins, outs)
        _lib.check(_lib.lib().o3dmi_pointcloud_select_by_mask(
            n, _lib.ptr(mask8), 0, len(group), a_in, widths, a_out,
            C.byref(m), stream()), "select_by_mask")
        for k, t in zip(group, outs):
            out[k] = t[:m.value]
    return out


def _selected(mesh, vertex_mask, tri_mask, triangles, n_tri, copy_attributes):
    """The mesh of a selection: positions and indices always, the other
    attributes with copy_attributes (CopyAttributesByMasks)."""
    vertex, triangle = _split(mesh)
    triangle.pop("indices", None)
    if not copy_attributes:
        vertex = {"positions": vertex["positions"]}
        triangle = {}
    out = _select_rows(vertex, vertex_mask)
    if "indices" in mesh:
        out.update(_select_rows(triangle, tri_mask))
        out["indices"] = triangles[:n_tri]
    return out


def select_faces_by_mask(mesh, mask):
    """TriangleMesh::SelectFacesByMask: the triangles with mask set, in input
    order, and the vertices they name, renumbered."""
    p = _positions(mesh)
    if "indices" not in mesh:
        return {}
    t = _indices(mesh, p)
    m = t.shape[0]
    mask = require_cuda(mask, "mask")
    if mask.dtype not in (torch.bool, torch.uint8) or mask.shape != (m,):
        raise ValueError("mask must be a bool {M} tensor")
    m8 = mask.view(torch.uint8)
    vmask = torch.empty(p.shape[0], dtype=torch.uint8, device=p.device)
    tris = torch.empty_like(t)
    n_tri, n_vert = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_select_faces_by_mask(
        *_index_args(p, t), _lib.ptr(m8), _lib.ptr(vmask), _lib.ptr(tris),
        C.byref(n_tri), C.byref(n_vert), stream()), "select_faces_by_mask")
    return _selected(mesh, vmask, m8, tris, n_tri.value, True)


def select_by_index(mesh, indices, copy_attributes=True):
    """TriangleMesh::SelectByIndex: the vertices named by `indices` (an index
    out of range is ignored, as upstream warns and continues) and the
    triangles all of whose vertices are kept. No index: the empty mesh."""
    p = _positions(mesh)
    indices = require_cuda(indices, "indices")
    if indices.dim() != 1 or indices.dtype not in (torch.int32, torch.int64):
        raise ValueError("indices must be an integer {K} tensor")
    if indices.shape[0] == 0:
        return {}
    indices = indices.to(torch.int64)
    t = _indices(mesh, p)
    vmask = torch.empty(p.shape[0], dtype=torch.uint8, device=p.device)
    tmask = torch.empty(t.shape[0], dtype=torch.uint8, device=p.device)
    tris = torch.empty_like(t)
    n_tri, n_vert, n_ign = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_select_by_index(
        *_index_args(p, t), _lib.ptr(indices), indices.shape[0],
        _lib.ptr(vmask), _lib.ptr(tmask), _lib.ptr(tris), C.byref(n_tri),
        C.byref(n_vert), C.byref(n_ign), stream()), "select_by_index")
    out = _selected(mesh, vmask, tmask, tris, n_tri.value, copy_attributes)
    if "indices" in out and n_tri.value == 0:
        # upstream sets no triangle indices when none survives
        out = {k: v for k, v in out.items()
               if k != "indices" and not k.startswith(TRIANGLE_PREFIX)}
    return out


def remove_unreferenced_vertices(mesh):
    """TriangleMesh::RemoveUnreferencedVertices: the vertices no triangle
    names leave; a mesh without triangles loses every vertex."""
    p = _positions(mesh)
    if p.shape[0] == 0:
        return dict(mesh)
    t = _indices(mesh, p)
    vmask = torch.empty(p.shape[0], dtype=torch.uint8, device=p.device)
    tris = torch.empty_like(t)
    n_vert = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_remove_unreferenced_vertices(
        *_index_args(p, t), _lib.ptr(vmask), _lib.ptr(tris), C.byref(n_vert),
        stream()), "remove_unreferenced_vertices")
    vertex, triangle = _split(mesh)
    out = _select_rows(vertex, vmask)
    out.update(triangle)
    if "indices" in mesh:
        out["indices"] = tris
    return out


def get_non_manifold_edges(mesh, allow_boundary_edges=True):
    """TriangleMesh::GetNonManifoldEdges -> {E,2} in the index dtype, in
    ascending (lo, hi) order (upstream: its hash map's order)."""
    p = _positions(mesh)
    t = _indices(mesh, p)
    args = _index_args(p, t) + (int(bool(allow_boundary_edges)),)
    n = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_get_non_manifold_edges(
        *args, None, -1, C.byref(n), stream()), "get_non_manifold_edges")
    edges = torch.empty((n.value, 2), dtype=t.dtype, device=p.device)
    if n.value:
        _lib.check(_lib.lib().o3dmi_trianglemesh_get_non_manifold_edges(
            *args, _lib.ptr(edges), n.value, C.byref(n), stream()),
            "get_non_manifold_edges")
    return edges


def cluster_connected_triangles(mesh):
    """Legacy TriangleMesh::ClusterConnectedTriangles -> (labels int32 {M},
    n_triangles int64 {C}, areas float64 {C}); clusters are numbered by their
    lowest triangle index, as upstream's loop numbers them."""
    p, t, args = _mesh_args(mesh)
    m = t.shape[0]
    labels = torch.empty(m, dtype=torch.int32, device=p.device)
    counts = torch.empty(m, dtype=torch.int64, device=p.device)
    areas = torch.empty(m, dtype=torch.float64, device=p.device)
    n = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_cluster_connected_triangles(
        *args, _lib.ptr(labels), C.byref(n), _lib.ptr(counts),
        _lib.ptr(areas), m, stream()), "cluster_connected_triangles")
    return labels, counts[:n.value], areas[:n.value]


# ---- clean-up, smoothing filters, vertex clustering ----------------------------

class FilterScope:
    """geometry::MeshBase::FilterScope."""
    All, Color, Normal, Vertex = 0, 1, 2, 3


class SimplificationContraction:
    """geometry::MeshBase::SimplificationContraction."""
    Average, Quadric = 0, 1


def remove_duplicated_vertices(mesh):
    """Legacy RemoveDuplicatedVertices: vertices with equal coordinates (by
    value: -0 == +0, a NaN row equals nothing) collapse onto the first of
    them; every vertex attribute keeps the first one's row and the triangles
    are renumbered."""
    p, t, args = _mesh_args(mesh)
    vmask = torch.empty(p.shape[0], dtype=torch.uint8, device=p.device)
    tris = torch.empty_like(t)
    n = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_remove_duplicated_vertices(
        *args, _lib.ptr(vmask), _lib.ptr(tris), C.byref(n), stream()),
        "remove_duplicated_vertices")
    vertex, triangle = _split(mesh)
    out = _select_rows(vertex, vmask)
    out.update(triangle)
    if "indices" in mesh:
        out["indices"] = tris
    return out


def _remove_triangles(mesh, call, what):
    p = _positions(mesh)
    if "indices" not in mesh:
        return dict(mesh)
    t = _indices(mesh, p)
    tmask = torch.empty(t.shape[0], dtype=torch.uint8, device=p.device)
    tris = torch.empty_like(t)
    n = C.c_int64(0)
    _lib.check(call(*_index_args(p, t), _lib.ptr(tmask), _lib.ptr(tris),
                    C.byref(n), stream()), what)
    vertex, triangle = _split(mesh)
    triangle.pop("indices")
    out = dict(vertex)
    out.update(_select_rows(triangle, tmask))
    out["indices"] = tris[:n.value]
    return out


def remove_duplicated_triangles(mesh):
    """Legacy RemoveDuplicatedTriangles: of the triangles that are rotations
    of one another the first stays (the flipped one is another triangle);
    triangle attributes follow."""
    return _remove_triangles(
        mesh, _lib.lib().o3dmi_trianglemesh_remove_duplicated_triangles,
        "remove_duplicated_triangles")


def remove_degenerate_triangles(mesh):
    """Legacy RemoveDegenerateTriangles: a triangle that names a vertex twice
    leaves; triangle attributes follow."""
    return _remove_triangles(
        mesh, _lib.lib().o3dmi_trianglemesh_remove_degenerate_triangles,
        "remove_degenerate_triangles")


def compute_adjacency_list(mesh):
    """Legacy ComputeAdjacencyList as CSR -> (row_splits int64 {V+1},
    neighbours in the index dtype): the neighbours of vertex u are
    neighbours[row_splits[u]:row_splits[u + 1]], ascending, without
    repeats."""
    p = _positions(mesh)
    t = _indices(mesh, p)
    args = _index_args(p, t)
    n = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_compute_adjacency_list(
        *args, None, None, -1, C.byref(n), stream()),
        "compute_adjacency_list")
    splits = torch.empty(p.shape[0] + 1, dtype=torch.int64, device=p.device)
    nbrs = torch.empty(n.value, dtype=t.dtype, device=p.device)
    _lib.check(_lib.lib().o3dmi_trianglemesh_compute_adjacency_list(
        *args, _lib.ptr(splits), _lib.ptr(nbrs), n.value, C.byref(n),
        stream()), "compute_adjacency_list")
    return splits, nbrs


def _vertex_attr(mesh, name, p):
    a = mesh.get(name)
    if a is None:
        return None
    a = require_cuda(a, name).contiguous()
    if a.shape != p.shape:
        raise ValueError("%s must be {V,3}" % name)
    return a


def _attr_args(p, normals, colors):
    """(normals, colors, attr_dtype) of a filter / clustering call."""
    given = [a for a in (normals, colors) if a is not None]
    dtypes = {a.dtype for a in given}
    if len(dtypes) > 1 or any(d not in TORCH_TO_O3DMI for d in dtypes):
        raise ValueError("normals and colors must have the position dtype")
    code = TORCH_TO_O3DMI[given[0].dtype] if given else TORCH_TO_O3DMI[p.dtype]
    return (_lib.ptr(normals), _lib.ptr(colors), code)


def _filter(mesh, call, params, scope, what):
    p, t, args = _mesh_args(mesh)
    p = p.contiguous()
    normals = _vertex_attr(mesh, "normals", p)
    colors = _vertex_attr(mesh, "colors", p)
    outs = [torch.empty_like(a) if a is not None else None
            for a in (p, normals, colors)]
    _lib.check(call(
        _lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype],
        *_attr_args(p, normals, colors), *args[3:], *params, int(scope),
        *[_lib.ptr(o) for o in outs], stream()), what)
    out = dict(mesh)
    for name, o in zip(("positions", "normals", "colors"), outs):
        if o is not None:
            out[name] = o
    return out


def filter_sharpen(mesh, number_of_iterations=1, strength=1.0,
                   filter_scope=FilterScope.All):
    """Legacy FilterSharpen: v_o = v_i + strength (v_i |N| - sum_N v_n) per
    iteration, in float64 over the neighbours in ascending index."""
    return _filter(mesh, _lib.lib().o3dmi_trianglemesh_filter_sharpen,
                   (int(number_of_iterations), float(strength)), filter_scope,
                   "filter_sharpen")


def filter_smooth_simple(mesh, number_of_iterations=1,
                         filter_scope=FilterScope.All):
    """Legacy FilterSmoothSimple: v_o = (v_i + sum_N v_n) / (|N| + 1)."""
    return _filter(mesh, _lib.lib().o3dmi_trianglemesh_filter_smooth_simple,
                   (int(number_of_iterations),), filter_scope,
                   "filter_smooth_simple")


def filter_smooth_laplacian(mesh, number_of_iterations=1, lambda_filter=0.5,
                            filter_scope=FilterScope.All):
    """Legacy FilterSmoothLaplacian with inverse-distance weights."""
    return _filter(mesh, _lib.lib().o3dmi_trianglemesh_filter_smooth_laplacian,
                   (int(number_of_iterations), float(lambda_filter)),
                   filter_scope, "filter_smooth_laplacian")


def filter_smooth_taubin(mesh, number_of_iterations=1, lambda_filter=0.5,
                         mu=-0.53, filter_scope=FilterScope.All):
    """Legacy FilterSmoothTaubin: a laplacian pass with lambda_filter, then
    one with mu, per iteration."""
    return _filter(mesh, _lib.lib().o3dmi_trianglemesh_filter_smooth_taubin,
                   (int(number_of_iterations), float(lambda_filter),
                    float(mu)), filter_scope, "filter_smooth_taubin")


def simplify_vertex_clustering(
        mesh, voxel_size, contraction=SimplificationContraction.Average):
    """Legacy SimplifyVertexClustering -> a mesh with "positions", "indices",
    "normals" / "colors" when the input has them, and "triangle_normals"
    recomputed when it had them. Clusters are numbered by their first
    vertex; the kept triangles stay in input order."""
    p, t, args = _mesh_args(mesh)
    p = p.contiguous()
    normals = _vertex_attr(mesh, "normals", p)
    colors = _vertex_attr(mesh, "colors", p)
    outs = [torch.empty_like(a) if a is not None else None
            for a in (p, normals, colors)]
    tris = torch.empty_like(t)
    n_v, n_t = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_simplify_vertex_clustering(
        _lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype],
        *_attr_args(p, normals, colors), *args[3:], float(voxel_size),
        int(contraction), *[_lib.ptr(o) for o in outs], _lib.ptr(tris),
        C.byref(n_v), C.byref(n_t), stream()), "simplify_vertex_clustering")
    out = {}
    for name, o in zip(("positions", "normals", "colors"), outs):
        if o is not None:
            out[name] = o[:n_v.value]
    if "indices" in mesh:
        out["indices"] = tris[:n_t.value]
    if TRIANGLE_PREFIX + "normals" in mesh:
        out = compute_triangle_normals(out, normalized=True)
    return out


def _subdivide(mesh, call, number_of_iterations, what):
    """The count call, the allocation, the call."""
    p, t, _ = _mesh_args(mesh)
    p = p.contiguous()
    t = t.contiguous()
    normals = _vertex_attr(mesh, "normals", p)
    colors = _vertex_attr(mesh, "colors", p)
    head = (_lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype],
            *_attr_args(p, normals, colors), _lib.ptr(t), t.shape[0],
            TORCH_TO_O3DMI[t.dtype], int(number_of_iterations))
    n_v, n_t = C.c_int64(0), C.c_int64(0)
    _lib.check(call(*head, None, None, None, -1, None, C.byref(n_v),
                    C.byref(n_t), stream()), what)
    outs = [torch.empty((n_v.value, 3), dtype=p.dtype, device=p.device)
            if a is not None else None for a in (p, normals, colors)]
    tris = torch.empty((n_t.value, 3), dtype=t.dtype, device=p.device)
    _lib.check(call(*head, *[_lib.ptr(o) for o in outs], n_v.value,
                    _lib.ptr(tris), C.byref(n_v), C.byref(n_t), stream()),
               what)
    out = {}
    for name, o in zip(("positions", "normals", "colors"), outs):
        if o is not None:
            out[name] = o
    if "indices" in mesh:
        out["indices"] = tris
    if TRIANGLE_PREFIX + "normals" in mesh:
        out = compute_triangle_normals(out, normalized=True)
    return out


def subdivide_midpoint(mesh, number_of_iterations=1):
    """Legacy SubdivideMidpoint -> a mesh with "positions", "indices",
    "normals" / "colors" when the input has them, and "triangle_normals"
    recomputed when it had them. Every triangle becomes four; the new vertex
    of an edge is the midpoint of its ends and is numbered in the order in
    which a walk over the triangles meets the edges first."""
    return _subdivide(mesh, _lib.lib().o3dmi_trianglemesh_subdivide_midpoint,
                      number_of_iterations, "subdivide_midpoint")


def subdivide_loop(mesh, number_of_iterations=1):
    """Legacy SubdivideLoop (Loop's masks with upstream's boundary rule), the
    same outputs and numbering as subdivide_midpoint. A vertex no triangle
    names is copied (upstream makes it NaN)."""
    return _subdivide(mesh, _lib.lib().o3dmi_trianglemesh_subdivide_loop,
                      number_of_iterations, "subdivide_loop")


# ---- ClipPlane / SlicePlane -----------------------------------------------------

def _vec3(x, name):
    """A list, a tuple or an int / float tensor of shape {3} -> 3 doubles."""
    if isinstance(x, torch.Tensor):
        if x.dtype == torch.bool or x.is_complex():
            raise ValueError("%s must be an int or float tensor" % name)
        x = x.detach().to("cpu", torch.float64).tolist()
    try:
        values = [float(e) for e in x]
    except TypeError:
        raise ValueError("%s must have shape {3}" % name) from None
    if len(values) != 3:
        raise ValueError("%s must have shape {3}" % name)
    return (C.c_double * 3)(*values)


def _cut_inputs(mesh, what):
    """-> positions, indices, the leading arguments of a clip / slice call, the
    kernel's attributes {name: tensor or None}, the other vertex attributes
    and the triangle attributes."""
    p, t, _ = _mesh_args(mesh)
    p = p.contiguous()
    t = t.contiguous()
    own = {"positions": p, "normals": _vertex_attr(mesh, "normals", p),
           "colors": _vertex_attr(mesh, "colors", p)}
    vertex, triangle = _split(mesh)
    triangle.pop("indices", None)
    extra = {}
    for name, a in vertex.items():
        if name in own:
            continue
        a = require_cuda(a, name)
        if not a.dtype.is_floating_point:
            raise ValueError(
                "%s: vertex attribute %r is not floating point and cannot be "
                "interpolated" % (what, name))
        if a.dim() < 1 or a.shape[0] != p.shape[0]:
            raise ValueError("attribute %r must have %d rows"
                             % (name, p.shape[0]))
        extra[name] = a
    for name, a in triangle.items():
        a = require_cuda(a, name)
        if a.dim() < 1 or a.shape[0] != t.shape[0]:
            raise ValueError("attribute %r must have %d rows"
                             % (name, t.shape[0]))
    head = (_lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype],
            *_attr_args(p, own["normals"], own["colors"]), _lib.ptr(t),
            t.shape[0], TORCH_TO_O3DMI[t.dtype])
    return p, t, head, own, extra, triangle


def _cut_outputs(own, rows):
    return {name: torch.empty((rows, 3), dtype=a.dtype, device=a.device)
            if a is not None else None for name, a in own.items()}


def _interpolate(a, source, t):
    """x_lo + t * (x_hi - x_lo) in float64 for the rows of a cut (two
    roundings, no fused multiply-add: the kernel's statement), the row of an
    old vertex as it is; narrowed to the attribute's dtype."""
    lo, hi = source[:, 0].long(), source[:, 1].long()
    w = a.to(torch.float64)
    x_lo, x_hi = w[lo], w[hi]
    tt = t.reshape((-1,) + (1,) * (a.dim() - 1))
    mixed = x_lo + torch.mul(tt, x_hi - x_lo)
    same = (lo == hi).reshape(tt.shape)
    return torch.where(same, x_lo, mixed).to(a.dtype)


def clip_plane(mesh, point, normal):
    """TriangleMesh::ClipPlane -> the part of the mesh with normal . (x -
    point) >= 0, as a pure function of the input (upstream: VTK). "positions",
    "normals" and "colors" go through the kernel; every other floating vertex
    attribute is interpolated by the same statement, x_lo + t (x_hi - x_lo) in
    float64 (a non-floating one raises ValueError); every "triangle_"
    attribute follows its input triangle. A triangle with one vertex inside
    becomes (a, ab, ca), one with two (a, b, bc), (a, bc, ca); a vertex on the
    plane is its own cut point; the kept old vertices come first, then the
    cut vertices in the order a walk over the output meets their edges.
    Coincident vertices are not merged (upstream merges them): call
    remove_duplicated_vertices first. point / normal: lists, tuples or int /
    float tensors of shape {3}; the normal is not normalised."""
    p, t, head, own, extra, triangle = _cut_inputs(mesh, "clip_plane")
    head += (_vec3(point, "point"), _vec3(normal, "normal"))
    call = _lib.lib().o3dmi_trianglemesh_clip_plane
    n_v, n_t = C.c_int64(0), C.c_int64(0)
    _lib.check(call(*head, None, None, None, -1, None, 0, None, None, None,
                    C.byref(n_v), C.byref(n_t), stream()), "clip_plane")
    outs = _cut_outputs(own, n_v.value)
    dev = p.device
    tris = torch.empty((n_t.value, 3), dtype=t.dtype, device=dev)
    tsrc = torch.empty(n_t.value, dtype=t.dtype, device=dev)
    vsrc = torch.empty((n_v.value, 2), dtype=t.dtype, device=dev)
    vt = torch.empty(n_v.value, dtype=torch.float64, device=dev)
    _lib.check(call(*head, *[_lib.ptr(outs[k]) for k in own], n_v.value,
                    _lib.ptr(tris), n_t.value, _lib.ptr(tsrc), _lib.ptr(vsrc),
                    _lib.ptr(vt), C.byref(n_v), C.byref(n_t), stream()),
               "clip_plane")
    out = {k: o for k, o in outs.items() if o is not None}
    for name, a in extra.items():
        out[name] = _interpolate(a, vsrc, vt)
    if "indices" in mesh:
        out["indices"] = tris
        rows = tsrc.long()
        for name, a in triangle.items():
            out[name] = a[rows]
    return out


def slice_plane(mesh, point, normal, contour_values=(0.0,)):
    """TriangleMesh::SlicePlane -> a line set dict: "positions" {P,3},
    "indices" {L,2}, the vertex attributes interpolated as in clip_plane,
    "line_triangle" {L} (the triangle of every line) and "line_contour" {L}
    int32. One line per crossed triangle and contour value c, from where the
    winding leaves normal . (x - point) >= c to where it re-enters; points are
    unique per contour, numbered contour after contour in the order a walk
    over the lines meets them. The normal is not normalised: c is in units of
    |normal| times distance. A triangle in the contour plane gives nothing;
    an in-plane edge is emitted by the triangle below it."""
    p, t, head, own, extra, _ = _cut_inputs(mesh, "slice_plane")
    values = [float(c) for c in contour_values]
    head += (_vec3(point, "point"), _vec3(normal, "normal"),
             (C.c_double * max(len(values), 1))(*values), len(values))
    call = _lib.lib().o3dmi_trianglemesh_slice_plane
    n_p, n_l = C.c_int64(0), C.c_int64(0)
    _lib.check(call(*head, None, None, None, -1, None, 0, None, None, None,
                    None, C.byref(n_p), C.byref(n_l), stream()),
               "slice_plane")
    outs = _cut_outputs(own, n_p.value)
    dev = p.device
    lines = torch.empty((n_l.value, 2), dtype=t.dtype, device=dev)
    ltri = torch.empty(n_l.value, dtype=t.dtype, device=dev)
    lcon = torch.empty(n_l.value, dtype=torch.int32, device=dev)
    psrc = torch.empty((n_p.value, 2), dtype=t.dtype, device=dev)
    pt = torch.empty(n_p.value, dtype=torch.float64, device=dev)
    _lib.check(call(*head, *[_lib.ptr(outs[k]) for k in own], n_p.value,
                    _lib.ptr(lines), n_l.value, _lib.ptr(ltri),
                    _lib.ptr(lcon), _lib.ptr(psrc), _lib.ptr(pt),
                    C.byref(n_p), C.byref(n_l), stream()), "slice_plane")
    out = {k: o for k, o in outs.items() if o is not None}
    for name, a in extra.items():
        out[name] = _interpolate(a, psrc, pt)
    out["indices"] = lines
    out["line_triangle"] = ltri
    out["line_contour"] = lcon
    return out


# ---- topology and intersection queries -----------------------------------------

def _contiguous_args(mesh):
    p = _positions(mesh).contiguous()
    t = _indices(mesh, p).contiguous()
    return p, t, (_lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype],
                  _lib.ptr(t), t.shape[0], TORCH_TO_O3DMI[t.dtype])


def euler_poincare_characteristic(mesh):
    """Legacy EulerPoincareCharacteristic: V + F - E, E the number of distinct
    (lo, hi) edges (a self edge of a repeated-vertex triangle counts)."""
    p, t, _ = _contiguous_args(mesh)
    chi = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_euler_poincare_characteristic(
        *_index_args(p, t), C.byref(chi), stream()),
        "euler_poincare_characteristic")
    return chi.value


def is_edge_manifold(mesh, allow_boundary_edges=True):
    """Legacy IsEdgeManifold: no edge of multiplicity > 2
    (allow_boundary_edges) or != 2."""
    p, t, _ = _contiguous_args(mesh)
    out = C.c_int(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_is_edge_manifold(
        *_index_args(p, t), int(bool(allow_boundary_edges)), C.byref(out),
        stream()), "is_edge_manifold")
    return bool(out.value)


def get_non_manifold_vertices(mesh):
    """Legacy GetNonManifoldVertices -> {N} in the index dtype, ascending: the
    vertices whose wedges' link edges form more than one connected component.
    A vertex named only by triangles that name it twice is not reported
    (upstream: undefined)."""
    p, t, _ = _contiguous_args(mesh)
    args = _index_args(p, t)
    n = C.c_int64(0)
    call = _lib.lib().o3dmi_trianglemesh_get_non_manifold_vertices
    _lib.check(call(*args, None, -1, C.byref(n), stream()),
               "get_non_manifold_vertices")
    out = torch.empty(n.value, dtype=t.dtype, device=p.device)
    if n.value:
        _lib.check(call(*args, _lib.ptr(out), n.value, C.byref(n), stream()),
                   "get_non_manifold_vertices")
    return out


def is_vertex_manifold(mesh):
    """Legacy IsVertexManifold."""
    p, t, _ = _contiguous_args(mesh)
    n = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_get_non_manifold_vertices(
        *_index_args(p, t), None, -1, C.byref(n), stream()),
        "is_vertex_manifold")
    return n.value == 0


def is_orientable(mesh):
    """Legacy IsOrientable, as a function of the mesh: an edge of
    multiplicity > 2 makes it false whatever the visiting order."""
    p, t, _ = _contiguous_args(mesh)
    ok = C.c_int(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_orient_triangles(
        *_index_args(p, t), None, C.byref(ok), stream()), "is_orientable")
    return bool(ok.value)


def orient_triangles(mesh):
    """Legacy OrientTriangles -> (mesh, orientable). When orientable, the
    lowest-indexed triangle of every connected component keeps its winding
    and a flipped (a, b, c) becomes (a, c, b); else "indices" is a copy.
    Only "indices" changes: normals are left alone, as upstream leaves
    them."""
    p, t, _ = _contiguous_args(mesh)
    out = dict(mesh)
    tris = torch.empty_like(t)
    ok = C.c_int(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_orient_triangles(
        *_index_args(p, t), _lib.ptr(tris), C.byref(ok), stream()),
        "orient_triangles")
    if "indices" in mesh:
        out["indices"] = tris
    return out, bool(ok.value)


def get_self_intersecting_triangles(mesh):
    """Legacy GetSelfIntersectingTriangles -> {N,2} in the index dtype, in
    ascending (i, j), i < j: the pairs that share no vertex index, whose
    float64 boxes overlap and that IntersectionTest::TriangleTriangle3d
    reports, found on the mesh BVH instead of upstream's all-pairs loop."""
    p, t, args = _contiguous_args(mesh)
    n = C.c_int64(0)
    call = _lib.lib().o3dmi_trianglemesh_get_self_intersecting_triangles
    _lib.check(call(*args, None, -1, C.byref(n), stream()),
               "get_self_intersecting_triangles")
    out = torch.empty((n.value, 2), dtype=t.dtype, device=p.device)
    if n.value:
        _lib.check(call(*args, _lib.ptr(out), n.value, C.byref(n), stream()),
                   "get_self_intersecting_triangles")
    return out


def is_self_intersecting(mesh):
    """Legacy IsSelfIntersecting."""
    _, _, args = _contiguous_args(mesh)
    out = C.c_int(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_is_self_intersecting(
        *args, C.byref(out), stream()), "is_self_intersecting")
    return bool(out.value)


def is_intersecting(mesh, other):
    """Legacy IsIntersecting: the bounding boxes of all vertices overlap and
    some triangle of `mesh` meets one of `other`. Unlike upstream every pair
    is box-tested first, so two nearly coplanar triangles with disjoint boxes
    never count."""
    _, _, args = _contiguous_args(mesh)
    _, _, other_args = _contiguous_args(other)
    out = C.c_int(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_is_intersecting(
        *args, *other_args, C.byref(out), stream()), "is_intersecting")
    return bool(out.value)


def is_watertight(mesh):
    """Legacy IsWatertight: edge manifold without boundary, vertex manifold
    and not self-intersecting, tested in that order."""
    _, _, args = _contiguous_args(mesh)
    out = C.c_int(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_is_watertight(
        *args, C.byref(out), stream()), "is_watertight")
    return bool(out.value)


def get_volume(mesh):
    """Legacy GetVolume: |sum of p0 . (p1 x p2) / 6| as a float64 sum in a
    fixed order; raises (upstream's messages) unless the mesh is watertight
    and orientable."""
    _, _, args = _contiguous_args(mesh)
    out = C.c_double(0)
    _lib.check(_lib.lib().o3dmi_trianglemesh_get_volume(
        *args, C.byref(out), stream()), "get_volume")
    return out.value


# ---- sampling, closest points, metrics ----------------------------------------

_COLOR_CODES = {torch.float32: 0, torch.uint8: 3, torch.uint16: 2}


def sample_points_uniformly(mesh, number_of_points, use_triangle_normal=False,
                            seed=0):
    """TriangleMesh::SamplePointsUniformly -> a point cloud dict: "positions",
    "normals" when the mesh has vertex normals (or use_triangle_normal: the
    triangle's normal, computed first if absent) and Float32 "colors" when it
    has vertex colors. Point j is a pure function of (mesh, seed, j); a
    triangle of area 0 is never drawn. Textures are not sampled."""
    p, t, args = _mesh_args(mesh)
    n = int(number_of_points)
    if n <= 0:
        raise ValueError("number_of_points <= 0")
    if p.shape[0] == 0:
        raise ValueError("Input mesh is empty. Cannot sample points.")
    if "indices" not in mesh or t.shape[0] == 0:
        raise ValueError("Input mesh has no triangles. Cannot sample points.")
    vn = tn = colors = None
    if use_triangle_normal:
        name = TRIANGLE_PREFIX + "normals"
        if name not in mesh:
            mesh = compute_triangle_normals(mesh, normalized=True)
        tn = require_cuda(mesh[name], name).to(p.dtype).contiguous()
        if tn.shape != (t.shape[0], 3):
            raise ValueError("triangle_normals must be {M,3}")
    elif "normals" in mesh:
        vn = require_cuda(mesh["normals"], "normals").to(p.dtype).contiguous()
        if vn.shape != p.shape:
            raise ValueError("normals must be {V,3}")
    if "colors" in mesh:
        colors = require_cuda(mesh["colors"], "colors")
        if colors.dtype not in _COLOR_CODES:
            colors = colors.to(torch.float32)
        colors = colors.contiguous()
        if colors.shape != p.shape:
            raise ValueError("colors must be {V,3}")
    out = {"positions": torch.empty((n, 3), dtype=p.dtype, device=p.device)}
    if vn is not None or tn is not None:
        out["normals"] = torch.empty((n, 3), dtype=p.dtype, device=p.device)
    if colors is not None:
        out["colors"] = torch.empty((n, 3), dtype=torch.float32,
                                    device=p.device)
    _lib.check(_lib.lib().o3dmi_trianglemesh_sample_points_uniformly(
        *args, n, int(seed) & (2 ** 64 - 1), _lib.ptr(vn), _lib.ptr(tn),
        _lib.ptr(colors),
        _COLOR_CODES[colors.dtype] if colors is not None else 0,
        _lib.ptr(out["positions"]), _lib.ptr(out.get("normals")),
        _lib.ptr(out.get("colors")), None, stream()),
        "sample_points_uniformly")
    return out


class MeshBVH:
    """The closest-point and ray queries of RaycastingScene for one triangle
    mesh (Float32): a linear BVH on the device that owns its copies of the
    mesh. The answer to a query is the minimum over all triangles, the lowest
    index on ties, whatever the tree."""

    def __init__(self, mesh):
        p, t, args = _mesh_args(mesh)
        handle = C.c_void_p()
        _lib.check(_lib.lib().o3dmi_mesh_bvh_create(
            *args, C.byref(handle), stream()), "MeshBVH")
        self._handle = handle
        self._device = p.device

    def close(self):
        if self._handle is not None:
            _lib.lib().o3dmi_mesh_bvh_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _queries(self, points):
        points = require_cuda(points, "query_points")
        if points.dim() < 1 or points.shape[-1] != 3:
            raise ValueError("query_points must have shape {..., 3}")
        return points.reshape(-1, 3).contiguous(), tuple(points.shape[:-1])

    def compute_closest_points(self, points):
        """-> dict(points {..,3}, geometry_ids {..} (all 0), primitive_ids
        {..} uint32, primitive_uvs {..,2}, primitive_normals {..,3}), as
        RaycastingScene::ComputeClosestPoints."""
        flat, lead = self._queries(points)
        q, dev = flat.shape[0], flat.device
        out = {
            "points": torch.empty((q, 3), dtype=torch.float32, device=dev),
            "primitive_ids": torch.empty(q, dtype=torch.uint32, device=dev),
            "primitive_uvs": torch.empty((q, 2), dtype=torch.float32,
                                         device=dev),
            "primitive_normals": torch.empty((q, 3), dtype=torch.float32,
                                             device=dev),
        }
        _lib.check(_lib.lib().o3dmi_mesh_bvh_closest_points(
            self._handle, _lib.ptr(flat), q, TORCH_TO_O3DMI[flat.dtype],
            _lib.ptr(out["points"]), _lib.ptr(out["primitive_ids"]),
            _lib.ptr(out["primitive_uvs"]),
            _lib.ptr(out["primitive_normals"]), None, stream()),
            "compute_closest_points")
        out["geometry_ids"] = torch.zeros(q, dtype=torch.uint32, device=dev)
        return {k: v.reshape(lead + tuple(v.shape[1:]))
                for k, v in out.items()}

    def compute_distance(self, points):
        """RaycastingScene::ComputeDistance -> {..} Float32."""
        flat, lead = self._queries(points)
        q = flat.shape[0]
        dist = torch.empty(q, dtype=torch.float32, device=flat.device)
        _lib.check(_lib.lib().o3dmi_mesh_bvh_closest_points(
            self._handle, _lib.ptr(flat), q, TORCH_TO_O3DMI[flat.dtype], None,
            None, None, None, _lib.ptr(dist), stream()), "compute_distance")
        return dist.reshape(lead)

    # ---- ray queries: pure functions of (mesh, ray), see the C header ------
    def _rays(self, rays):
        rays = require_cuda(rays, "rays")
        if rays.dim() < 1 or rays.shape[-1] != 6:
            raise ValueError("rays must have shape {..., 6}")
        return rays.reshape(-1, 6).contiguous(), tuple(rays.shape[:-1])

    def cast_rays(self, rays):
        """RaycastingScene::CastRays -> dict(t_hit {..}, geometry_ids {..},
        primitive_ids {..} uint32, primitive_uvs {..,2}, primitive_normals
        {..,3}): the smallest t, the lowest triangle index among equals; a
        miss is t_hit inf and INVALID_ID."""
        flat, lead = self._rays(rays)
        q, dev = flat.shape[0], flat.device
        out = {
            "t_hit": torch.empty(q, dtype=torch.float32, device=dev),
            "geometry_ids": torch.empty(q, dtype=torch.uint32, device=dev),
            "primitive_ids": torch.empty(q, dtype=torch.uint32, device=dev),
            "primitive_uvs": torch.empty((q, 2), dtype=torch.float32,
                                         device=dev),
            "primitive_normals": torch.empty((q, 3), dtype=torch.float32,
                                             device=dev),
        }
        _lib.check(_lib.lib().o3dmi_mesh_bvh_cast_rays(
            self._handle, _lib.ptr(flat), q, TORCH_TO_O3DMI[flat.dtype],
            _lib.ptr(out["t_hit"]), _lib.ptr(out["geometry_ids"]),
            _lib.ptr(out["primitive_ids"]), _lib.ptr(out["primitive_uvs"]),
            _lib.ptr(out["primitive_normals"]), stream()), "cast_rays")
        return {k: v.reshape(lead + tuple(v.shape[1:]))
                for k, v in out.items()}

    def test_occlusions(self, rays, tnear=0.0, tfar=float("inf")):
        """RaycastingScene::TestOcclusions -> {..} bool: whether anything is
        hit on (tnear, tfar]."""
        flat, lead = self._rays(rays)
        q = flat.shape[0]
        out = torch.empty(q, dtype=torch.uint8, device=flat.device)
        _lib.check(_lib.lib().o3dmi_mesh_bvh_test_occlusions(
            self._handle, _lib.ptr(flat), q, TORCH_TO_O3DMI[flat.dtype],
            float(tnear), float(tfar), _lib.ptr(out), stream()),
            "test_occlusions")
        return out.to(torch.bool).reshape(lead)

    def count_intersections(self, rays):
        """RaycastingScene::CountIntersections -> {..} int32: the number of
        distinct t at which the ray meets the mesh."""
        flat, lead = self._rays(rays)
        q = flat.shape[0]
        out = torch.empty(q, dtype=torch.int32, device=flat.device)
        _lib.check(_lib.lib().o3dmi_mesh_bvh_count_intersections(
            self._handle, _lib.ptr(flat), q, TORCH_TO_O3DMI[flat.dtype],
            _lib.ptr(out), stream()), "count_intersections")
        return out.reshape(lead)

    def list_intersections(self, rays):
        """RaycastingScene::ListIntersections -> dict(ray_splits {R+1} int64,
        ray_ids {N} int64, t_hit {N}, geometry_ids {N}, primitive_ids {N}
        uint32, primitive_uvs {N,2}), the entries of a ray in ascending t."""
        flat, _ = self._rays(rays)
        q, dev = flat.shape[0], flat.device
        splits = torch.empty(q + 1, dtype=torch.int64, device=dev)
        total = C.c_int64(0)
        head = (self._handle, _lib.ptr(flat), q, TORCH_TO_O3DMI[flat.dtype],
                _lib.ptr(splits))
        _lib.check(_lib.lib().o3dmi_mesh_bvh_list_intersections(
            *head, -1, C.byref(total), None, None, None, None, None,
            stream()), "list_intersections")
        n = total.value
        out = {
            "ray_splits": splits,
            "ray_ids": torch.empty(n, dtype=torch.int64, device=dev),
            "t_hit": torch.empty(n, dtype=torch.float32, device=dev),
            "geometry_ids": torch.empty(n, dtype=torch.uint32, device=dev),
            "primitive_ids": torch.empty(n, dtype=torch.uint32, device=dev),
            "primitive_uvs": torch.empty((n, 2), dtype=torch.float32,
                                         device=dev),
        }
        if n:
            _lib.check(_lib.lib().o3dmi_mesh_bvh_list_intersections(
                *head, n, C.byref(total), _lib.ptr(out["ray_ids"]),
                _lib.ptr(out["t_hit"]), _lib.ptr(out["geometry_ids"]),
                _lib.ptr(out["primitive_ids"]),
                _lib.ptr(out["primitive_uvs"]), stream()),
                "list_intersections")
        return out

    def compute_occupancy(self, points, nsamples=1):
        """RaycastingScene::ComputeOccupancy -> {..} Float32, 1 inside and 0
        outside by the vote of nsamples (odd) rays per point."""
        flat, lead = self._queries(points)
        q = flat.shape[0]
        out = torch.empty(q, dtype=torch.float32, device=flat.device)
        _lib.check(_lib.lib().o3dmi_mesh_bvh_compute_occupancy(
            self._handle, _lib.ptr(flat), q, TORCH_TO_O3DMI[flat.dtype],
            int(nsamples), _lib.ptr(out), stream()), "compute_occupancy")
        return out.reshape(lead)

    def compute_signed_distance(self, points, nsamples=1):
        """RaycastingScene::ComputeSignedDistance -> {..} Float32: the
        distance, negative inside."""
        flat, lead = self._queries(points)
        q = flat.shape[0]
        out = torch.empty(q, dtype=torch.float32, device=flat.device)
        _lib.check(_lib.lib().o3dmi_mesh_bvh_compute_signed_distance(
            self._handle, _lib.ptr(flat), q, TORCH_TO_O3DMI[flat.dtype],
            int(nsamples), _lib.ptr(out), stream()),
            "compute_signed_distance")
        return out.reshape(lead)


INVALID_ID = 0xFFFFFFFF  # RaycastingScene::INVALID_ID


def create_rays_pinhole(intrinsic, extrinsic, width, height, device="cuda"):
    """RaycastingScene::CreateRaysPinhole -> {height, width, 6} Float32 rays
    on the device from a 3x3 intrinsic and a 4x4 extrinsic matrix (host
    tensors or nested lists)."""
    # nested lists of Python floats are doubles: not through torch's float32
    k = torch.as_tensor(intrinsic, dtype=torch.float64).detach().cpu()
    e = torch.as_tensor(extrinsic, dtype=torch.float64).detach().cpu()
    if tuple(k.shape) != (3, 3) or tuple(e.shape) != (4, 4):
        raise ValueError("intrinsic must be {3,3} and extrinsic {4,4}")
    k, e = k.contiguous(), e.contiguous()
    width, height = int(width), int(height)
    if width <= 0 or height <= 0:
        raise ValueError("width and height must be positive")
    rays = torch.empty((height, width, 6), dtype=torch.float32, device=device)
    _lib.check(_lib.lib().o3dmi_create_rays_pinhole(
        C.cast(k.data_ptr(), C.POINTER(C.c_double)),
        C.cast(e.data_ptr(), C.POINTER(C.c_double)), width, height,
        _lib.ptr(rays), stream()), "create_rays_pinhole")
    return rays


def compute_metrics(mesh1, mesh2, metrics, fscore_radius=(0.01,),
                    n_sampled_points=1000, seed=0, return_raw=False):
    """TriangleMesh::ComputeMetrics -> a CPU Float32 tensor with the values in
    the order of `metrics` (pointcloud.Metric codes; every FScore entry expands
    to one value per radius). Mesh 1 is sampled with `seed`, mesh 2 with
    seed + 1. With return_raw also dict(sum, max, counts), each with the
    direction 1 -> 2 first. Float32 meshes."""
    p1, t1, _ = _mesh_args(mesh1)
    p2, t2, _ = _mesh_args(mesh2)
    if p1.dtype != p2.dtype:
        raise ValueError("both meshes must have the same dtype")
    codes = [int(m) for m in metrics]
    radii = [float(r) for r in fscore_radius]
    n_values = sum(len(radii) if m == _pc.Metric.FScore else 1 for m in codes)
    values = (C.c_float * max(n_values, 1))()
    counts = (C.c_int64 * max(2 * len(radii), 1))()
    raw = _lib.MetricsRawC()
    raw.counts = C.cast(counts, C.POINTER(C.c_int64))
    _lib.check(_lib.lib().o3dmi_trianglemesh_compute_metrics(
        _lib.ptr(p1), p1.shape[0], _lib.ptr(t1), t1.shape[0],
        TORCH_TO_O3DMI[t1.dtype], _lib.ptr(p2), p2.shape[0], _lib.ptr(t2),
        t2.shape[0], TORCH_TO_O3DMI[t2.dtype], TORCH_TO_O3DMI[p1.dtype],
        (C.c_int * max(len(codes), 1))(*codes), len(codes),
        (C.c_float * max(len(radii), 1))(*radii), len(radii),
        int(n_sampled_points), int(seed) & (2 ** 64 - 1), values, n_values,
        C.byref(raw), stream()), "compute_metrics")
    out = torch.tensor(list(values)[:n_values], dtype=torch.float32)
    if not return_raw:
        return out
    r = len(radii)
    return out, dict(sum=list(raw.sum), max=list(raw.max),
                     counts=[list(counts)[:r], list(counts)[r:2 * r]])


def compute_convex_hull(mesh, joggle_inputs=False):
    """TriangleMesh::ComputeConvexHull: the hull of the vertex positions, as
    pointcloud.compute_convex_hull returns it (joggle_inputs=True raises
    ValueError there)."""
    return _pc.compute_convex_hull({"positions": _positions(mesh)},
                                   joggle_inputs)


def get_oriented_bounding_box(mesh, robust=False, method="minimal_approx"):
    """TriangleMesh::GetOrientedBoundingBox: the box of the vertex positions,
    as pointcloud.get_oriented_bounding_box returns it."""
    _pc._refuse_robust(robust)
    return _pc.get_oriented_bounding_box({"positions": _positions(mesh)},
                                         robust, method)


def get_oriented_bounding_ellipsoid(mesh, robust=False):
    """TriangleMesh::GetOrientedBoundingEllipsoid: the ellipsoid of the vertex
    positions, as pointcloud.get_oriented_bounding_ellipsoid returns it."""
    _pc._refuse_robust(robust)
    return _pc.get_oriented_bounding_ellipsoid(
        {"positions": _positions(mesh)}, robust)
